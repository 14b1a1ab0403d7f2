"""Host mirror of the device generator (mmvae_philox_* of csrc/elbo_optim.hip): Philox4x32-10 in plain numpy, the
uniform / keep-mask arithmetic bit for bit in float32, the normal draw in float64.  No GPU, no project import.

Word layout of the kernels: counter words c0, c1 = low / high half of the 64-bit counter (offset + q), c2, c3 = low /
high half of the stream id, key words k0, k1 = low / high half of the seed.  Element 4q + j of a fill is word j of
philox(offset + q)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # key bumps
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_U64 = (1 << 64) - 1
TWO_PI_F32 = np.float32(6.283185307179586)


def philox_rounds(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32 over counter words c0..c3 (arrays or scalars below 2^32) and key words k0, k1: four uint32 arrays.
    All arithmetic in uint64, masked to 32 bits."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & _LO for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n1 = p1 & _LO
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        n3 = p0 & _LO
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def philox4x32_10(counter_u64, stream_u64, seed_u64):
    """Four uint32 arrays, vectorised over `counter` (uint64 array or int); `stream` and `seed` are ints below 2^64."""
    counter = np.atleast_1d(np.asarray(counter_u64, dtype=np.uint64))
    stream, seed = int(stream_u64) & _U64, int(seed_u64) & _U64
    return philox_rounds(counter & _LO, counter >> _S32, stream & 0xFFFFFFFF, stream >> 32, seed & 0xFFFFFFFF, seed >> 32)


def counters(n, offset):
    """The (n + 3) // 4 counters of an n-element fill at `offset` (wraps modulo 2^64 like the device's uint64 sum)."""
    return np.uint64(int(offset) & _U64) + np.arange((int(n) + 3) // 4, dtype=np.uint64)


def words(n, seed, offset, stream):
    """[(n + 3) // 4, 4] uint32: row q is philox(offset + q)."""
    return np.stack(philox4x32_10(counters(n, offset), stream, seed), axis=1)


def u01(w):
    """The kernel's uniform, in its order of operations: ((float)(w >> 8) + 0.5f) * 2^-24, in [2^-25, 1.0]."""
    w = np.asarray(w, dtype=np.uint32)
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def keep_mask(n, p, seed, offset, stream):
    """uint8[n]: 1 where u01 >= float32(p)."""
    u = u01(words(n, seed, offset, stream)).reshape(-1)[:n]
    return (u >= np.float32(p)).astype(np.uint8)


def normal_from_words(w):
    """w [..., 4] uint32 -> (values, radii), both float64 [..., 4]: r0 cos0, r0 sin0, r1 cos1, r1 sin1 with r0 from u0,
    its angle from u1, r1 from u2, its angle from u3.  The angle is the float32 product 2 pi * u the kernel hands to
    sincosf; log, sqrt, sin and cos are float64."""
    u = u01(w)
    r = np.sqrt(-2.0 * np.log(u[..., 0::2].astype(np.float64)))           # [..., 2]: r0, r1
    a = (TWO_PI_F32 * u[..., 1::2]).astype(np.float32).astype(np.float64)  # [..., 2]: angle 0, angle 1
    vals = np.stack([r[..., 0] * np.cos(a[..., 0]), r[..., 0] * np.sin(a[..., 0]),
                     r[..., 1] * np.cos(a[..., 1]), r[..., 1] * np.sin(a[..., 1])], axis=-1)
    radii = np.stack([r[..., 0], r[..., 0], r[..., 1], r[..., 1]], axis=-1)
    return vals, radii


def normal_with_radius(n, seed, offset, stream):
    """(float64[n] standard normals, float64[n] Box-Muller radius of each element)."""
    vals, radii = normal_from_words(words(n, seed, offset, stream))
    return vals.reshape(-1)[:n], radii.reshape(-1)[:n]


def normal(n, seed, offset, stream):
    """float64[n]: the fill of mmvae_philox_normal in float64."""
    return normal_with_radius(n, seed, offset, stream)[0]
