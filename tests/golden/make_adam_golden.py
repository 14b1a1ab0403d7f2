#!/usr/bin/env python3
"""Record what the by-value Adam entry points of ABI 13 computed: tests/golden/adam_by_value.npz.

ABI 14 removed mmvae_adam_step, mmvae_adam_step_copy, mmvae_adam_step_jobs and mmvae_adam_step_multi; their `_hp` forms
stay and tests/test_optim_hyper_gpu.py holds those to the bits recorded here.  Needs a GPU and a libmmvae_hip.so built
from the last ABI 13 commit (9bd20b9):

    MMVAE_LIB=/path/to/abi13/libmmvae_hip.so python tests/golden/make_adam_golden.py

The library is bound here with plain ctypes (the package's binding no longer knows the retired symbols); the inputs are
the test module's own builders (seeded CPU generators).  In the same run every by-value result is compared with what
the ABI 13 `_hp` entry gives for hyper = {lr, wd, 0, 0}: the file is written only when both families agree bit for bit,
so it is what either produced at that commit.
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

OUT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT_DIR))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_optim_hyper_gpu as T  # noqa: E402

_i, _l, _f, _p = C.c_int, C.c_int64, C.c_float, C.c_void_p
SIGNATURES = {
    "mmvae_abi_version": [],
    "mmvae_adam_set_workgroups": [_i],
    # retired with ABI 14
    "mmvae_adam_step": [_l, _p, _p, _p, _p, _p, _f, _f, _f, _f, _f, _f, _p],
    "mmvae_adam_step_copy": [_l, _p, _p, _p, _p, _p, _f, _f, _f, _f, _f, _f, _i, _p, _p, _p],
    "mmvae_adam_step_jobs": [_i, _p, _p, _p, _p, _p, _p, _f, _f, _f, _f, _f, _f, _p],
    "mmvae_adam_step_multi": [_i, _p, _l, _p],
    # their ABI 13 siblings
    "mmvae_adam_step_hp": [_l, _p, _p, _p, _p, _p, _p, _f, _f, _f, _f, _p],
    "mmvae_adam_step_copy_hp": [_l, _p, _p, _p, _p, _p, _p, _f, _f, _f, _f, _i, _p, _p, _p],
    "mmvae_adam_step_jobs_hp": [_i, _p, _p, _p, _p, _p, _p, _p, _f, _f, _f, _f, _p],
    "mmvae_adam_step_multi_hp": [_i, _p, _l, _p],
}


class ArenaByValue(C.Structure):  # mmvae_adam_arena of ABI 13
    _fields_ = [("p", _p), ("g", _p), ("m", _p), ("v", _p), ("state", _p), ("n", _l), ("lr", _f), ("beta1", _f),
                ("beta2", _f), ("eps", _f), ("weight_decay", _f), ("grad_scale", _f)]


class ArenaHp(C.Structure):  # mmvae_adam_arena_hp
    _fields_ = [("p", _p), ("g", _p), ("m", _p), ("v", _p), ("state", _p), ("hyper", _p), ("n", _l), ("beta1", _f),
                ("beta2", _f), ("eps", _f), ("grad_scale", _f)]


def ptrs(ts):
    return [t.data_ptr() for t in ts]


def same(a, b, what):
    for x, y in zip(a, b):
        assert torch.equal(x, y), f"ABI 13 by-value and _hp results differ: {what}"


def main():
    lib = C.CDLL(os.environ["MMVAE_LIB"])
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _i, args
    abi = lib.mmvae_abi_version()
    if abi != 13:
        raise SystemExit(f"{os.environ['MMVAE_LIB']}: ABI {abi}; the by-value entries are recorded from ABI 13 only")
    assert torch.cuda.is_available()
    LR, WD, B1, B2, EPS, GS = T.LR, T.WD, T.B1, T.B2, T.EPS, T.GS
    s = T._stream()
    out = {}

    # the step: 16-byte body + tail, the scalar path of an unaligned arena, fewer than 4 elements.  One record per offset:
    # at ABI 13 the 16-byte loop and the scalar loop of the same kernel do not round alike (seen on an MI355X).
    for n, offsets in ((4099, (0, 1)), (3, (0,))):
        for cv in (0.0, 0.05):
            state = T._state(cv)
            for off in offsets:
                ref, got = T._arenas(n, off), T._arenas(n, off)
                a = T._views(ref, n, off)
                assert lib.mmvae_adam_step(n, *ptrs(a), state.data_ptr(), LR, B1, B2, EPS, WD, GS, s) == 0
                b = T._views(got, n, off)
                assert lib.mmvae_adam_step_hp(n, *ptrs(b), state.data_ptr(), T._hyper().data_ptr(), B1, B2, EPS, GS, s) == 0
                torch.cuda.synchronize()
                same(ref, got, f"step n={n} offset={off} cv={cv}")
                for name, t in zip("pgmv", a):
                    if name != "g":
                        out[f"step_n{n}_off{off}_cv{cv:g}_{name}"] = t.clone()
                assert not torch.equal(a[0], T._views(T._arenas(n, off), n, off)[0])

    # the copy rider, chip-filling and confined grids: the bits of the plain step at n = 4099, cv = 0
    n, state, src = 4099, T._state(), T._rnd(256, 5).cuda()
    try:
        for wg in (0, 7):
            assert lib.mmvae_adam_set_workgroups(wg) == 0
            for hp in (False, True):
                a, dst = T._arenas(n), torch.zeros(256, device="cuda")
                if hp:
                    rc = lib.mmvae_adam_step_copy_hp(n, *ptrs(a), state.data_ptr(), T._hyper().data_ptr(), B1, B2, EPS, GS,
                                                     256, src.data_ptr(), dst.data_ptr(), s)
                else:
                    rc = lib.mmvae_adam_step_copy(n, *ptrs(a), state.data_ptr(), LR, B1, B2, EPS, WD, GS, 256,
                                                  src.data_ptr(), dst.data_ptr(), s)
                assert rc == 0
                torch.cuda.synchronize()
                assert torch.equal(dst, src)
                same([out[f"step_n{n}_off0_cv0_{k}"] for k in "pmv"], [a[0][:n], a[2][:n], a[3][:n]], f"copy wg={wg} hp={hp}")
    finally:
        lib.mmvae_adam_set_workgroups(0)

    # the job list
    n, jobs_dev, state = T.JOB_N, T._job_table(), T._state()
    ref, got = T._arenas(n), T._arenas(n)
    assert lib.mmvae_adam_step_jobs(len(T.JOB_SEGS), jobs_dev.data_ptr(), *ptrs(ref), state.data_ptr(), LR, B1, B2, EPS,
                                    WD, GS, s) == 0
    assert lib.mmvae_adam_step_jobs_hp(len(T.JOB_SEGS), jobs_dev.data_ptr(), *ptrs(got), state.data_ptr(),
                                       T._hyper().data_ptr(), B1, B2, EPS, GS, s) == 0
    torch.cuda.synchronize()
    same(ref, got, "jobs")
    for name, t in zip("pgmv", ref):
        if name != "g":
            out[f"jobs_{name}"] = t[:n]

    # several arenas in one launch
    sizes = T.MULTI_SIZES
    states = [T._state(cv) for cv in T.MULTI_CV]
    hypers = [T._hyper(lr, wd) for _, _, lr, wd in sizes]
    results = []
    for hp in (False, True):
        arenas = [T._arenas(n, off) for n, off, _, _ in sizes]
        table = ((ArenaHp if hp else ArenaByValue) * len(sizes))()
        for e, full, (n, off, lr, wd), st, hy in zip(table, arenas, sizes, states, hypers):
            e.p, e.g, e.m, e.v = ptrs(T._views(full, n, off))
            e.state, e.n = st.data_ptr(), n
            e.beta1, e.beta2, e.eps, e.grad_scale = B1, B2, EPS, GS
            if hp:
                e.hyper = hy.data_ptr()
            else:
                e.lr, e.weight_decay = lr, wd
        raw = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
        fn = lib.mmvae_adam_step_multi_hp if hp else lib.mmvae_adam_step_multi
        assert fn(len(sizes), raw.data_ptr(), max(n for n, _, _, _ in sizes), s) == 0
        torch.cuda.synchronize()
        results.append(arenas)
    for k, (ref, got, (n, off, _, _)) in enumerate(zip(results[0], results[1], sizes)):
        same(ref, got, f"multi arena {k}")
        for name, t in zip("pgmv", T._views(ref, n, off)):
            if name != "g":
                out[f"multi{k}_{name}"] = t

    arrays = {k: v.cpu().numpy() for k, v in out.items()}
    assert all(a.dtype == np.float32 for a in arrays.values())
    path = os.path.join(os.environ.get("MMVAE_GOLDEN_OUT", OUT_DIR), "adam_by_value.npz")
    np.savez_compressed(path, **arrays)
    print(f"by-value == _hp at ABI 13 for every case; wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
