"""The conditional-layer kernels of mmvae_amd/csrc/cond_layers.hip restated in numpy: every cell goes through the Linear of
its own condition block, the blocks lie in one arena and are addressed by per-block element offsets, as the kernels do.

    forward      y[j, b]  = W[c_j(b)] x[j, b] + bias[c_j(b)]                          for positions j = 0 .. n_pos - 1
    input_grad   dx[b]    = sum over positions j (descending) of W[c_j(b)]^T dy[j, b]  (+ the old dx with `old`)
    weight_grad  dW[c]    = sum over the cells of c, in batch order, of dy[b] (x) x[b],  db[c] = sum dy[b]
                 for the blocks present in the batch only; every other float of the gradient arena is NaN

One position is n_pos = 1 (2-D arguments are taken as that).  In float64 these are the reference (held to a per-condition
torch loop with autograd in tests/test_cond_layers_host.py).  Each returns, beside the value, S: the same expression with
every operand replaced by its absolute value (|bias| and |old dx| included) -- the magnitude a float32 evaluation's error
scales with: any order of a float32 sum of n products, contracted or not, deviates by at most (n + 3) 2^-24 S.

The *_f32 functions evaluate the same statements in float32 in the kernels' documented summation order (products rounded,
then added): lane-strided partial sums over 64 lanes and a halving tree for y; two chains over the halves of the output
rows, added, positions in descending order for dx; a chain in cell order inside chunks of 32 cells with the chunk
partials added in piece order for dW.  The host test uses them to show that the bound has room and that integer data is
exact."""
import numpy as np

U = 2.0 ** -24   # unit roundoff of float32
CHUNK = 32       # cells per piece of a block's weight gradient (MMVAE_COND_DW_CHUNK)
LANES = 64


def block(arena, off, c, *shape):
    n = int(np.prod(shape))
    return arena[int(off[c]):int(off[c]) + n].reshape(shape)


def _positions(a, cond):
    """cond as [n_pos, B]; a as [n_pos, B, width] (one shared [B, width] input is repeated)"""
    cond = np.atleast_2d(np.asarray(cond))
    a = np.asarray(a)
    if a.ndim == 2:
        a = np.broadcast_to(a, (cond.shape[0],) + a.shape)
    assert a.shape[:2] == cond.shape
    return a, cond


def bound(n, S):
    """|float32 sum of n products - exact| <= (n + 3) 2^-24 S, per element"""
    return (np.asarray(n, np.float64) + 3.0) * U * S


# ------------------------------------------------------------------------------------------------------------ float64
def forward(x, arena, w_off, b_off, cond, n_out):
    """-> y, S of shape [n_pos, B, n_out]"""
    x, cond = _positions(x, cond)
    n_pos, B, n_in = x.shape
    y, S = np.zeros((n_pos, B, n_out)), np.zeros((n_pos, B, n_out))
    for j in range(n_pos):
        for c in np.unique(cond[j]):
            sel = cond[j] == c
            W = block(arena, w_off, c, n_out, n_in).astype(np.float64)
            bias = block(arena, b_off, c, n_out).astype(np.float64)
            xs = x[j, sel].astype(np.float64)
            y[j, sel] = xs @ W.T + bias
            S[j, sel] = np.abs(xs) @ np.abs(W).T + np.abs(bias)
    return y, S


def input_grad(dy, arena, w_off, cond, n_in, old=None):
    """-> dx, S of shape [B, n_in]; `old`: the dx that an accumulating call adds to"""
    dy, cond = _positions(dy, cond)
    n_pos, B, n_out = dy.shape
    dx, S = np.zeros((B, n_in)), np.zeros((B, n_in))
    for j in range(n_pos - 1, -1, -1):
        for c in np.unique(cond[j]):
            sel = cond[j] == c
            W = block(arena, w_off, c, n_out, n_in).astype(np.float64)
            g = dy[j, sel].astype(np.float64)
            dx[sel] += g @ W
            S[sel] += np.abs(g) @ np.abs(W)
    if old is not None:
        dx += np.asarray(old, np.float64)
        S += np.abs(np.asarray(old, np.float64))
    return dx, S


def weight_grad(dy, x, cond, w_off, b_off, size):
    """-> G, S, n: gradient arenas of `size` floats -- NaN outside the present blocks -- and the number of cells summed into
    each element (0 outside).  The positions' blocks are distinct (cond holds global block indices)."""
    dy, cond = _positions(dy, cond)
    x, _ = _positions(x, cond)
    n_out, n_in = dy.shape[2], x.shape[2]
    G, S, n = np.full(size, np.nan), np.full(size, np.nan), np.zeros(size, np.int64)
    for j in range(cond.shape[0]):
        for c in np.unique(cond[j]):
            sel = cond[j] == c
            g, xs = dy[j, sel].astype(np.float64), x[j, sel].astype(np.float64)
            for arr, a, b in ((G, g, xs), (S, np.abs(g), np.abs(xs))):
                block(arr, w_off, c, n_out, n_in)[:] = a.T @ b
                block(arr, b_off, c, n_out)[:] = a.sum(0)
            block(n, w_off, c, n_out, n_in)[:] = int(sel.sum())
            block(n, b_off, c, n_out)[:] = int(sel.sum())
    return G, S, n


# ------------------------------------------------------------------------------------------------------------ float32
def forward_f32(x, arena, w_off, b_off, cond, n_out):
    x, cond = _positions(x, cond)
    n_pos, B, n_in = x.shape
    y = np.zeros((n_pos, B, n_out), np.float32)
    for j in range(n_pos):
        for c in np.unique(cond[j]):
            sel = cond[j] == c
            W = block(arena, w_off, c, n_out, n_in).astype(np.float32)
            xs = x[j, sel].astype(np.float32)
            lanes = np.zeros((xs.shape[0], n_out, LANES), np.float32)   # lane l: k = l, l + 64, ... in order
            for k0 in range(0, n_in, LANES):
                w = min(LANES, n_in - k0)
                lanes[:, :, :w] += W[None, :, k0:k0 + w] * xs[:, None, k0:k0 + w]
            m = LANES // 2
            while m >= 1:                                                # the butterfly as lane 0 sees it
                lanes = lanes[:, :, :m] + lanes[:, :, m:2 * m]
                m //= 2
            y[j, sel] = lanes[:, :, 0] + block(arena, b_off, c, n_out).astype(np.float32)
    return y


def input_grad_f32(dy, arena, w_off, cond, n_in, old=None):
    dy, cond = _positions(dy, cond)
    n_pos, B, n_out = dy.shape
    mid = (n_out + 1) // 2
    dx = np.zeros((B, n_in), np.float32)
    for j in range(n_pos - 1, -1, -1):
        v = np.zeros((B, n_in), np.float32)
        for c in np.unique(cond[j]):
            sel = cond[j] == c
            W = block(arena, w_off, c, n_out, n_in).astype(np.float32)
            g = dy[j, sel].astype(np.float32)
            halves = []
            for lo, hi in ((0, mid), (mid, n_out)):
                acc = np.zeros((g.shape[0], n_in), np.float32)
                for o in range(lo, hi):
                    acc += W[o][None, :] * g[:, o:o + 1]
                halves.append(acc)
            v[sel] = halves[0] + halves[1]
        dx = v if j == n_pos - 1 else dx + v
    if old is not None:
        dx = np.asarray(old, np.float32) + dx
    return dx


def weight_grad_f32(dy, x, cond, w_off, b_off, size):
    dy, cond = _positions(dy, cond)
    x, _ = _positions(x, cond)
    n_out, n_in = dy.shape[2], x.shape[2]
    G = np.full(size, np.nan, np.float32)
    for j in range(cond.shape[0]):
        for c in np.unique(cond[j]):
            cells = np.flatnonzero(cond[j] == c)                         # batch order
            dW, db = None, None
            for beg in range(0, len(cells), CHUNK):
                pw, pb = np.zeros((n_out, n_in), np.float32), np.zeros(n_out, np.float32)
                for b in cells[beg:beg + CHUNK]:
                    g, xs = dy[j, b].astype(np.float32), x[j, b].astype(np.float32)
                    pw += g[:, None] * xs[None, :]
                    pb += g
                dW, db = (pw, pb) if dW is None else (dW + pw, db + pb)
            block(G, w_off, c, n_out, n_in)[:] = dW
            block(G, b_off, c, n_out)[:] = db
    return G
