"""Cases and restatement for the batch-norm kernels' documented summation order (include/ucnerf_hip.h, "batch-statistic batch-norm", SUMMATION
ORDER), shared by tests/test_bn_order_host.py (CPU) and tests/test_hip_bn_order.py (GPU).

The restatement is numpy, written from the header's words and sharing no code with the package: per slice the thread chunks (a left-to-right
float64 sum, mean = sum / count, a left-to-right M2), the thread's chain of Chan merges over its chunks, the six lane steps, the sixteen waves
ascending; then the apply launch's fold over the P slices, ONE rounding of mu and M2 / N to float32 and the float32 epilogue with an exactly
rounded fmaf (rays_cases.fma32).  Everything is vectorised over channels, slices, threads and chunks; `trim` drops whole waves and chunk
positions that hold no value in any slice, which are no-ops by the header's "b empty -> a" (the host test shows trim on and off give the same
bits).  The library is compiled without contraction and with IEEE division and square root, so the device's bits are expected."""
import math

import numpy as np

from rays_cases import fma32

F32, F64 = np.float32, np.float64
THREADS, CHUNK_QUADS, LANES = 1024, 4, 64                # the header's numbers: 1024 threads, chunks of 4 quads, waves of 64 lanes
WAVES = THREADS // LANES
ROUND = THREADS * 4                                      # values one round of the block covers: a thread's quads lie 4096 values apart
CHUNK = CHUNK_QUADS * ROUND                              # values one chunk of every thread covers
MIN_SLICE, MAX_PARTIALS, APPLY_BLOCK = 4096, 32, 4096
EPS, MOMENTUM = 1e-5, 0.1
GUARD = 64

# the measured distance of the restatement's triples from the exact ones over CASES (test_bn_order_host.py prints it; profiles/bn_order.md),
# relative to the exact value; the bar is 4 x this, at least one float64 spacing of the largest value.  The GPU file falls back to that bar
# only where a bit comparison had to be relaxed for a named reason (none had to).
MEASURED_MEAN_REL, MEASURED_M2_REL = 3.6e-16, 6.2e-16    # (measured 3.59e-16 at n3_s43691 and 6.13e-16 at n2_s131072, rounded up)


# ------------------------------------------------------------------------------------------------ the header's partition
def partials(N):
    return min(MAX_PARTIALS, -(-N // MIN_SLICE))


def slice_length(N, P):
    return (-(-N // P) + 3) // 4 * 4


def slice_counts(N):
    """-> (P, L, the P slice lengths) by the header's formula."""
    P = partials(N)
    L = slice_length(N, P)
    return P, L, [min((j + 1) * L, N) - j * L for j in range(P)]


def regime(n, S):
    """What a shape reaches, from the header's formulas alone."""
    N = n * S
    P, L, counts = slice_counts(N)
    quads = -(-counts[0] // 4)                                            # of slice 0, the longest
    return dict(N=N, P=P, L=L, last=counts[-1], quads=quads, chunks=-(-quads // (CHUNK_QUADS * THREADS)),
                live_u=min(CHUNK_QUADS, -(-quads // THREADS)),               # rounds of chunk 0 that hold a value: u = 0 .. live_u - 1
                threads_u1=min(max(quads - THREADS, 0), THREADS),            # threads whose u = 1 quad of chunk 0 lies in slice 0
                second_chunk_quads=max(quads - CHUNK_QUADS * THREADS, 0),
                empty_threads=max(THREADS - quads, 0), last_quad=(counts[-1] - 1) % 4 + 1, vec=S % 4 == 0)


# ------------------------------------------------------------------------------------------------ the cases
# name -> (n, C, S, what the row claims of regime(n, S))
CASES = {
    "n2_s1": (2, 3, 1, dict(N=2, P=1, L=4, empty_threads=1023, last_quad=2)),
    "s2": (1, 3, 2, dict(N=2, P=1, L=4, empty_threads=1023, last_quad=2)),
    "s3": (1, 2, 3, dict(N=3, P=1, L=4, empty_threads=1023, last_quad=3)),
    "s5": (1, 3, 5, dict(N=5, P=1, L=8, empty_threads=1022, last_quad=1)),
    "s4095": (1, 2, 4095, dict(P=1, L=4096, last=4095, quads=1024, empty_threads=0, last_quad=3, live_u=1)),
    "s4096": (1, 3, 4096, dict(P=1, L=4096, last=4096, quads=1024, empty_threads=0, last_quad=4, live_u=1, vec=True)),
    "s4097": (1, 3, 4097, dict(P=2, L=2052, last=2045, last_quad=1, live_u=1)),
    "ragged": (2, 3, 4097, dict(N=8194, P=3, L=2732, last=2730, live_u=1)),
    "s131072": (1, 2, 131072, dict(P=32, L=4096, last=4096, quads=1024, live_u=1, threads_u1=0, chunks=1, vec=True)),
    "s131073": (1, 2, 131073, dict(P=32, L=4100, last=3973, live_u=2, threads_u1=1, chunks=1, vec=False)),
    "n3_s43691": (3, 2, 43691, dict(N=131073, P=32, L=4100, last=3973, live_u=2, threads_u1=1, chunks=1, vec=False)),
    "s131076": (1, 2, 131076, dict(P=32, L=4100, last=3976, live_u=2, threads_u1=1, chunks=1, vec=True)),
    "n2_s131072": (2, 2, 131072, dict(N=262144, P=32, L=8192, last=8192, live_u=2, threads_u1=1024, chunks=1, vec=True)),
    "s524288": (1, 2, 524288, dict(P=32, L=16384, last=16384, quads=4096, live_u=4, chunks=1, second_chunk_quads=0, vec=True)),
    "s524292": (1, 2, 524292, dict(P=32, L=16388, last=16264, live_u=4, chunks=2, second_chunk_quads=1, vec=True)),
    "n3_s174763": (3, 2, 174763, dict(N=524289, P=32, L=16388, last=16261, live_u=4, chunks=2, second_chunk_quads=1, last_quad=1, vec=False)),
    "c65535": (2, 65535, 1, dict(N=2, P=1, L=4)),
    # beyond the issue's table: every thread merges a FULL second chunk into its run.  In the two rows above only thread 0 of a slice does, with
    # 4 values of 16 388, which no bit of the slice's triple shows (the host test measures 0 of 64 against the "chunk64" order).
    "s1048576": (1, 1, 1048576, dict(P=32, L=32768, last=32768, live_u=4, chunks=2, second_chunk_quads=4096, vec=True)),
}
BIG = ("s524288", "s524292", "n3_s174763", "s1048576")   # the rows the order alternatives are told apart on
GUARDED = ("s4097", "n3_s43691", "s524292")              # the rows of the nothing-outside-the-extent test
CONDITIONING = ("s524292", "n3_s174763")
LAYOUT_N = 8200                                          # (4, 2050): 2050 is no multiple of 4


def seed_of(name):
    return 7000 + list(CASES).index(name)


_cache = {}


def data(name):
    """The inputs of a case, read-only: y and skip [n,C,S], gamma, beta, running_mean, running_var [C]; every channel its own contents."""
    if name not in _cache:
        n, C, S, _ = CASES[name]
        g = np.random.default_rng(seed_of(name))
        d = dict(y=(1.5 * g.standard_normal((n, C, S)) + 0.5 + 0.25 * np.arange(C)[None, :, None]).astype(F32),
                 skip=g.standard_normal((n, C, S)).astype(F32), gamma=(0.6 + 0.8 * g.random(C)).astype(F32),
                 beta=(0.3 * g.standard_normal(C)).astype(F32), rm=(0.3 * g.standard_normal(C)).astype(F32), rv=(0.5 + 1.5 * g.random(C)).astype(F32))
        for v in d.values():
            v.setflags(write=False)
        _cache[name] = d
    return _cache[name]


def channels(y):
    """[n,C,S] -> [C,N], a channel's values in the header's numbering i = img * S + offset."""
    n, C, S = y.shape
    return np.ascontiguousarray(np.transpose(y, (1, 0, 2))).reshape(C, n * S)


# ------------------------------------------------------------------------------------------------ the restatement: stats
def merge(a, b):
    """Chan's pairwise update as the header gives it, on tuples (n, mean, M2) of float64 arrays: b empty -> a."""
    na, ma, qa = a
    nb, mb, qb = b
    with np.errstate(all="ignore"):
        n = na + nb
        r = nb / n
        d = mb - ma
        mean = ma + d * r
        m2 = (qa + qb) + (d * d) * (na * r)
    empty = nb == 0.0
    return np.where(empty, na, n), np.where(empty, ma, mean), np.where(empty, qa, m2)


def partition(N, trim=True):
    """-> (idx, valid) of shape [P, K, T, 16]: the index i of the e-th value of quad u (position 4 u + e) of chunk k of thread t of slice j, and
    whether it lies inside the slice.  T is 1024, K the chunks of the longest slice; with `trim`, T stops at the last wave and the positions at
    the last one that holds a value in any slice."""
    P, L, _ = slice_counts(N)
    K = -(-L // CHUNK)
    j, k, t = np.arange(P)[:, None, None, None, None], np.arange(K)[None, :, None, None, None], np.arange(THREADS)[None, None, :, None, None]
    u, e = np.arange(CHUNK_QUADS)[None, None, None, :, None], np.arange(4)[None, None, None, None, :]
    local = ((CHUNK_QUADS * k + u) * THREADS + t) * 4 + e                 # quad (4 k + u) 1024 + t at j L + 4 q
    idx = (j * L + local).reshape(P, K, THREADS, 16)
    valid = ((local < L) & (j * L + local < N)).reshape(P, K, THREADS, 16)
    if trim:
        T = -(-(int(np.nonzero(valid.any((0, 1, 3)))[0].max()) + 1) // LANES) * LANES
        E = int(np.nonzero(valid.any((0, 1, 2)))[0].max()) + 1
        idx, valid = idx[:, :, :T, :E], valid[:, :, :T, :E]
    return idx, valid


def by_threads(x, N, T=THREADS, E=16):
    """The values x [C, N] laid out as partition() numbers them, [C, P, K, T, E], by slicing and reshaping (zeros outside the slices): what
    x[:, idx] gathers, without the gather (the host test compares the two).  T and E: the trimmed sizes."""
    P, L, counts = slice_counts(N)
    K = -(-L // CHUNK)
    if K == 1 and E <= 4:                                                  # every value in a u = 0 quad: position 4 t + e of its slice
        xp = np.zeros((x.shape[0], P, 4 * T), x.dtype)
        for j in range(P):
            xp[:, j, :counts[j]] = x[:, j * L:j * L + counts[j]]
        return xp.reshape(-1, P, 1, T, 4)[..., :E]
    xp = np.zeros((x.shape[0], P, K * CHUNK), x.dtype)
    for j in range(P):
        xp[:, j, :counts[j]] = x[:, j * L:j * L + counts[j]]
    return xp.reshape(-1, P, K, CHUNK_QUADS, THREADS, 4).transpose(0, 1, 2, 4, 3, 5).reshape(-1, P, K, THREADS, 16)[:, :, :, :T, :E]


def regroup(a, order):
    """[.., K, T, 16] in the chunks of an alternative order: "chunk8" [.., 2 K, T, 8], "chunk64" [.., K / 4, T, 64] (K padded with empty chunks)."""
    lead, (K, T, E) = a.shape[:-3], a.shape[-3:]
    if order == "chunk8":
        return np.moveaxis(a.reshape(lead + (K, T, 2, 8)), -2, -3).reshape(lead + (2 * K, T, 8))
    if order == "chunk64":
        a = np.concatenate([a, np.zeros(lead + (-K % 4, T, E), a.dtype)], -3)
        return np.moveaxis(a.reshape(lead + (-1, 4, T, E)), -3, -2).reshape(lead + (-1, T, 4 * E))
    return a


def thread_chunks(v, valid):
    """-> the chunk triples [C, P, K, T] of the values v [C, P, K, T, E], `valid` [P, K, T, E] of them inside their slice."""
    v = np.where(valid[None], v.astype(F64), 0.0)                            # (a value outside the slice is never added: + 0.0 is exact)
    cnt = valid.sum(-1).astype(F64)[None] + np.zeros(v.shape[:-1])
    with np.errstate(all="ignore"):
        s = np.zeros(v.shape[:-1])
        for p in range(v.shape[-1]):
            s = s + v[..., p]
        mean = s / cnt
        m2 = np.zeros(v.shape[:-1])
        for p in range(v.shape[-1]):
            d = np.where(valid[None, ..., p], v[..., p] - mean, 0.0)
            m2 = m2 + d * d
    return cnt, np.where(cnt == 0, 0.0, mean), np.where(cnt == 0, 0.0, m2)


def lanes_and_waves(run, order="documented"):
    """Thread triples [..., T] -> the block's triple [...]: six lane steps on the values of before each step, then the waves ascending."""
    lead = run[0].shape[:-1]
    run = tuple(a.reshape(lead + (-1, LANES)) for a in run)
    lane = np.arange(LANES)
    if order == "lane_scan":                                               # (an alternative: lane 0 takes lanes 1 .. 63 one after the other)
        acc = tuple(a[..., 0] for a in run)
        for l in range(1, LANES):
            acc = merge(acc, tuple(a[..., l] for a in run))
        wave = acc
    else:
        for d in (1, 2, 4, 8, 16, 32):
            src = np.minimum(lane + d, LANES - 1)
            new = merge(run, tuple(a[..., src] for a in run))
            run = tuple(np.where(lane + d < LANES, b, a) for a, b in zip(run, new))
        wave = tuple(a[..., 0] for a in run)
    W = wave[0].shape[-1]
    seq = range(W - 1, -1, -1) if order == "waves_descending" else range(W)
    acc = None
    for w in seq:
        b = tuple(a[..., w] for a in wave)
        acc = b if acc is None else merge(acc, b)
    return acc


def stats(y, trim=True, order="documented"):
    """ucnerf_bn_stats restated: y [n,C,S] float32 -> the workspace [C, P, 3] float64.  `order`: "documented", or one of the alternatives the
    host test tells it from: "waves_descending", "lane_scan", "chunk64" (one chunk of 64 values in place of four of 16; the same thing where a
    thread has one chunk) and "chunk8" (chunks of two quads)."""
    y = np.asarray(y, dtype=F32)
    n, C, S = y.shape
    N = n * S
    x = channels(y)
    idx, valid = partition(N, trim and order not in ("chunk64", "chunk8"))
    T, E = valid.shape[2:]
    valid = regroup(valid, order)
    per = max(1, (1 << 22) // (valid.size if E <= 4 else max(valid.size, valid.shape[0] * -(-N // valid.shape[0] // CHUNK) * CHUNK)))     # channels per pass: about 4 M values
    out = np.empty((C,) + valid.shape[:1] + (3,), F64)
    for c0 in range(0, C, per):
        ch = thread_chunks(regroup(by_threads(x[c0:c0 + per], N, T, E), order), valid)
        run = tuple(np.zeros(ch[0].shape[:2] + ch[0].shape[3:]) for _ in range(3))       # empty
        for k in range(valid.shape[1]):
            run = merge(run, tuple(a[:, :, k] for a in ch))
        for i, a in enumerate(lanes_and_waves(run, order)):
            out[c0:c0 + per, :, i] = a
    return out


# ------------------------------------------------------------------------------------------------ the restatement: apply
def fold(ws):
    """[C, P, 3] -> (n, mean, M2) [C]: merge(.. merge(triple 0, triple 1) .., triple P - 1)."""
    acc = tuple(ws[:, 0, i] for i in range(3))
    for j in range(1, ws.shape[1]):
        acc = merge(acc, tuple(ws[:, j, i] for i in range(3)))
    return acc


def apply(y, ws, gamma, beta, rm, rv, relu=True, skip=None, eps=EPS, momentum=MOMENTUM):
    """ucnerf_bn_apply restated -> dict(out [n,C,S], saved_mean, saved_var, running_mean, running_var [C]), all float32."""
    y = np.asarray(y, dtype=F32)
    cnt, mean, m2 = fold(np.asarray(ws, dtype=F64))
    with np.errstate(all="ignore"):
        mu, var, unbiased = mean.astype(F32), (m2 / cnt).astype(F32), (m2 / (cnt - 1.0)).astype(F32)     # each rounded once
        s = np.asarray(gamma, F32) / np.sqrt(var + F32(eps))
        r = fma32(y - mu[None, :, None], s[None, :, None], np.asarray(beta, F32)[None, :, None])
        if relu:
            r = np.where(r < 0, F32(0), r)                                 # (a NaN stays, and so does -0)
        if skip is not None:
            r = r + np.asarray(skip, F32)
        m = F32(momentum)
        new_rm = (F32(1) - m) * np.asarray(rm, F32) + m * mu
        new_rv = (F32(1) - m) * np.asarray(rv, F32) + m * unbiased
    assert r.dtype == F32 and new_rm.dtype == F32 and new_rv.dtype == F32 and s.dtype == F32
    return dict(out=r, saved_mean=mu, saved_var=var, running_mean=new_rm, running_var=new_rv)


def restate(name, relu=True, skip=False):
    """A case's workspace and every output, by the documented order (the workspace is computed once per case)."""
    d = data(name)
    key = (name, "ws")
    if key not in _cache:
        _cache[key] = stats(d["y"])
        _cache[key].setflags(write=False)
    out = apply(d["y"], _cache[key], d["gamma"], d["beta"], d["rm"], d["rv"], relu=relu, skip=d["skip"] if skip else None)
    out["workspace"] = _cache[key]
    return out


NAMES = ("workspace", "saved_mean", "saved_var", "running_mean", "running_var", "out")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == F64 else np.int32)


def first_difference(name, got, want):
    """None where the two arrays have the same bits, otherwise a line that names the first differing position and both values."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "%s: shape / dtype %s %s against %s %s" % (name, got.shape, got.dtype, want.shape, want.dtype)
    bad = bits(got) != bits(want)
    if not bad.any():
        return None
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    where = "(channel, slice, count|mean|M2)" if name == "workspace" else "(image, channel, offset)" if got.ndim == 3 else "(channel)"
    return "%s: %d of %d differ, first at %s = %s: device %r, restatement %r" % (name, int(bad.sum()), bad.size, where, at, got[at].item(), want[at].item())


# ------------------------------------------------------------------------------------------------ one value, every edge
def one_value_positions(n, S):
    """The positions i of the one-value test for a shape, sorted: the ends, the first and last value of slices 0, 1 and P - 1, either side of
    every 1024-quad round boundary inside a slice (quads 1023 | 1024, .. 4095 | 4096 of slices 0 and P - 1), of an image boundary and of the
    apply launch's first block edge."""
    N = n * S
    P, L, counts = slice_counts(N)
    want = {0, N - 1, APPLY_BLOCK - 1, APPLY_BLOCK}
    for j in {0, min(1, P - 1), P - 1}:
        want |= {j * L, j * L + counts[j] - 1}
        for q in range(THREADS, -(-counts[j] // 4) + 1, THREADS):          # quad q - 1 | quad q
            want |= {j * L + 4 * q - 1, j * L + 4 * q}
    for img in range(1, n):
        want |= {img * S - 1, img * S}
    return sorted(i for i in want if 0 <= i < N)


def one_value(n, S, positions):
    """[n, len(positions), S] of zeros with channel c holding 1.0 at its position."""
    x = np.zeros((len(positions), n * S), F32)
    x[np.arange(len(positions)), positions] = 1.0
    return np.ascontiguousarray(x.reshape(len(positions), n, S).transpose(1, 0, 2))


# ------------------------------------------------------------------------------------------------ the exact yardstick of the host test
def exact_triples(y):
    """[n,C,S] -> (mean, M2) [C, P] of every slice in extended precision: math.fsum for the sum (exact, rounded once), then numpy.longdouble
    two-pass for M2 where longdouble is wider than float64, math.fsum over the float64 squares otherwise."""
    x = channels(np.asarray(y, F32)).astype(F64)
    C, N = x.shape
    P, L, counts = slice_counts(N)
    wide = np.finfo(np.longdouble).nmant > 52
    mean, m2 = np.empty((C, P), np.longdouble), np.empty((C, P), np.longdouble)
    for c in range(C):
        for j in range(P):
            v = x[c, j * L:j * L + counts[j]]
            if wide:
                vl = v.astype(np.longdouble)
                mean[c, j] = vl.sum() / np.longdouble(counts[j])              # (pairwise in 64-bit mantissas: 2^-11 of float64's spacing)
                m2[c, j] = ((vl - mean[c, j]) ** 2).sum()
            else:
                mean[c, j] = math.fsum(v) / counts[j]
                m2[c, j] = math.fsum((v - F64(mean[c, j])) ** 2)
    return mean, m2


def spacing64(v):
    return 2.0 ** (math.floor(math.log2(max(float(v), 1e-300))) - 52)


# ------------------------------------------------------------------------------------------------ conditioning inputs
def conditioning(kind, n, C, S, seed):
    """-> y [n,C,S] float32: "offset" 1000 + 0.01 randn; "ramp" 100 i / N + noise (slice means differ by far more than sigma: Chan's
    (d d)(na r) term carries the variance); "constant_slice" slice 1 of every channel constant, the rest random."""
    N = n * S
    g = np.random.default_rng(seed)
    if kind == "offset":
        x = 1000.0 + 0.01 * g.standard_normal((C, N))
    elif kind == "ramp":
        x = 100.0 * np.arange(N)[None] / N + (0.5 + np.arange(C))[:, None] * g.standard_normal((C, N))
    else:
        P, L, _ = slice_counts(N)
        x = 1.5 * g.standard_normal((C, N)) + 0.5
        x[:, L:2 * L] = 2.5 + np.arange(C)[:, None]
    return np.ascontiguousarray(x.astype(F32).reshape(C, n, S).transpose(1, 0, 2))
