# Bench line + rocprofv3 kernel stats for the configurations beside the headline (run on the GPU box from the repo root):
# tools/collect_config_profiles.sh TAG [OUT]  ->  OUT/TAG_bench_line_<cfg>.json, TAG_kernel_stats_<cfg>.csv (c3, c4, c5,
# the reference's gene counts, the conditional model), TAG_configs.jsonl (tools/bench_all_configs.sh); OUT defaults to
# profile_out.  The bench runs take --full: the lines carry their own roofline (and C4's parity) blocks.
tag=$1
out=${2:-profile_out}
root=$PWD
cd /tmp && export TMPDIR=/tmp && cd $root
mkdir -p $out
for cfg in c3 c4 c5; do
  python3 bench.py --config $cfg --full --no-cpu-baseline > $out/${tag}_bench_line_${cfg}.json 2> $out/${tag}_bench_${cfg}.err || exit 1
  rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_${tag}_${cfg} -o b -- python3 bench.py --config $cfg --steps 30 --warmup 6 --full --no-cpu-baseline --no-parity > $out/${tag}_bench_under_rocprof_${cfg}.json 2>> $out/${tag}_bench_${cfg}.err || exit 1
  cp $(find $out/prof_${tag}_${cfg} -name "*kernel_stats.csv" | head -1) $out/${tag}_kernel_stats_${cfg}.csv
  rm -rf $out/prof_${tag}_${cfg}
done
python3 bench.py --genes 60530,52437 --full --no-cpu-baseline --no-parity > $out/${tag}_bench_line_refgenes.json 2> $out/${tag}_bench_refgenes.err || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_${tag}_refgenes -o b -- python3 bench.py --genes 60530,52437 --steps 30 --warmup 6 --full --no-cpu-baseline --no-parity > /dev/null 2>> $out/${tag}_bench_refgenes.err || exit 1
cp $(find $out/prof_${tag}_refgenes -name "*kernel_stats.csv" | head -1) $out/${tag}_kernel_stats_refgenes.csv
rm -rf $out/prof_${tag}_refgenes
# the conditional model: sequential selection order, then the reference's default ("parallel") with str and with categorical metadata
python3 tools/bench_conditional.py --engine-only 2> $out/${tag}_conditional.err | tail -1 > $out/${tag}_conditional.txt || exit 1
python3 tools/bench_conditional.py --engine-only --categorical 2>> $out/${tag}_conditional.err | tail -1 | sed 's/captured engine     :/captured engine, sequential order, categorical metadata:/' >> $out/${tag}_conditional.txt || exit 1
python3 tools/bench_conditional.py --parallel 2>> $out/${tag}_conditional.err | tail -1 >> $out/${tag}_conditional.txt || exit 1
python3 tools/bench_conditional.py --parallel --categorical 2>> $out/${tag}_conditional.err | tail -1 >> $out/${tag}_conditional.txt || exit 1
python3 tools/time_conditional_host.py --parallel 2>> $out/${tag}_conditional.err | tail -2 >> $out/${tag}_conditional.txt || exit 1
python3 tools/time_conditional_host.py --parallel --categorical 2>> $out/${tag}_conditional.err | tail -2 >> $out/${tag}_conditional.txt || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_${tag}_cond -o b -- python3 tools/bench_conditional.py --parallel > /dev/null 2>> $out/${tag}_conditional.err || exit 1
cp $(find $out/prof_${tag}_cond -name "*kernel_stats.csv" | head -1) $out/${tag}_kernel_stats_conditional.csv
rm -rf $out/prof_${tag}_cond
bash tools/bench_all_configs.sh > $out/${tag}_configs.jsonl
cat $out/${tag}_configs.jsonl
