"""Shared inputs of tests/test_batch_sample_host.py and tests/test_gpu_batch_sample.py: the NumPy twin of k_batch_sample
-- the walk shot by shot with ``trajectories.sample_uniform``, a fast form vectorised over the shots that draws the same
configurations, the margin of every decision, the dense probabilities of a list of cores -- and the cases of the device
tests with the seeds that the host test shows to be safe: every decision at least MARGIN away from its boundary, so that
the rounding of a g_j (a few ulp) cannot turn one."""

import numpy as np

from . import jump_oracle as jo
from . import spectra_cases as sc

SHAPES = sc.SHAPES  # "mixed", "odd", "wide": partial tiles in M, N and K of wg_gemm; K = 40: three K steps, d dr = 80: three N tiles
random_states = sc.random_states

CHUNK = 64       # BATCH_SAMPLE_CHUNK
MARGIN = 1e-6    # the least |u G - running sum| / G the device tests' inputs may have
B, NSHOTS = 3, 150  # 150 = 64 + 64 + 22: two full chunks and a partial one
# name -> (seed of the states, seed of the request); chosen so that every decision has margin >= MARGIN (asserted in
# tests/test_batch_sample_host.py)
CASES = {"mixed": (30, 1), "odd": (30, 1), "wide": (30, 1)}
# the statistical case: "mixed", two states, 4096 shots each; seeds chosen so that the twin keeps the 4.5 sigma bars
STAT = dict(name="mixed", B=2, nshots=4096, state_seed=70, seed=1, sigmas=4.5, pair=(1, 3))

_M64 = np.uint64((1 << 64) - 1)


def _mix(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniforms(seed, trajectory_id, step, nsite, nshots):
    """(nshots, nsite) array of sample_uniform(seed, trajectory_id, step, site, shot), in uint64 arithmetic"""
    with np.errstate(over="ignore"):
        base = _mix(_mix(np.uint64(seed) ^ np.uint64(trajectory_id)) + np.uint64(step))
        site = _mix(base + np.arange(nsite, dtype=np.uint64))
        key = _mix(site[None, :] + np.arange(nshots, dtype=np.uint64)[:, None])
    return (key >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def pick(g, u):
    """the selection rule of bc_pick on the weights g: G in index order, the smallest j whose running sum exceeds u G,
    else the last j with g_j > 0; -1 when G == 0.  Returns (j, G, margin) with margin = min_j |u G - running sum_j| / G."""
    G = 0.0
    for x in g:
        G += x
    if not G > 0.0:
        return -1, 0.0, np.inf
    thr = u * G
    j, last, run, margin = -1, 0, 0.0, np.inf
    for k, x in enumerate(g):
        run += x
        if x > 0.0:
            last = k
        if j < 0 and run > thr:
            j = k
        margin = min(margin, abs(thr - run) / G)
    return (last if j < 0 else j), G, margin


def walk(cores, nshots, seed, trajectory_id, step):
    """the contract, shot by shot: configs (nshots, L) int32, prob (nshots,), margins (nshots, L)"""
    from pytdscf_amd.trajectories import sample_uniform

    L = len(cores)
    configs = np.full((nshots, L), -1, dtype=np.int32)
    prob = np.zeros(nshots)
    margins = np.full((nshots, L), np.inf)
    for t in range(nshots):
        v, pr = np.ones(1, dtype=np.complex128), 1.0
        for p, C in enumerate(cores):
            w = np.tensordot(v, C, axes=(0, 0))  # (d, dr)
            g = [float(np.sum(np.abs(row) ** 2)) for row in w]
            j, G, margins[t, p] = pick(g, sample_uniform(seed, trajectory_id, step, p, t))
            if j < 0:
                pr = 0.0
                break
            configs[t, p] = j
            v = w[j] / np.sqrt(g[j])
            pr *= g[j] / G
        prob[t] = pr
    return configs, prob, margins


def walk_fast(cores, nshots, seed, trajectory_id, step):
    """the same walk with all shots at once (what a host would run): one matrix product per site.  Returns configs, prob
    and margins as ``walk`` does; the running sums are cumsum's, in index order."""
    L = len(cores)
    u = uniforms(seed, trajectory_id, step, L, nshots)
    configs = np.full((nshots, L), -1, dtype=np.int32)
    prob = np.ones(nshots)
    margins = np.full((nshots, L), np.inf)
    alive = np.ones(nshots, dtype=bool)
    V = np.ones((nshots, 1), dtype=np.complex128)
    rows = np.arange(nshots)
    for p, C in enumerate(cores):
        dl, d, dr = C.shape
        W = (V @ C.reshape(dl, d * dr)).reshape(nshots, d, dr)
        g = np.sum(W.real ** 2 + W.imag ** 2, axis=2)
        run = np.cumsum(g, axis=1)
        G = run[:, -1]
        alive &= G > 0.0
        thr = u[:, p] * G
        over = run > thr[:, None]
        j = over.argmax(axis=1)
        lastpos = d - 1 - (g[:, ::-1] > 0.0).argmax(axis=1)
        j = np.where(over.any(axis=1), j, lastpos)
        Gs = np.where(alive, G, 1.0)
        gj = np.where(alive, g[rows, j], 1.0)
        margins[:, p] = np.where(alive, np.abs(thr[:, None] - run).min(axis=1) / Gs, np.inf)
        configs[:, p] = np.where(alive, j, -1)
        prob = np.where(alive, prob * gj / Gs, 0.0)
        V = np.where(alive[:, None], W[rows, j, :] / np.sqrt(gj)[:, None], 0.0)
    return configs, prob, margins


def dense_probs(cores):
    """|<j_0 .. j_{L-1}|psi>|^2 / <psi|psi> of the state of a list of cores, shaped by the physical dimensions"""
    v = jo.dense_state(cores)
    p = np.abs(v) ** 2
    return (p / p.sum()).reshape([c.shape[1] for c in cores])


def histogram(configs, dims):
    """freq as the kernel forms it: per site the counts of every outcome, (double) count / (double) nshots"""
    n = configs.shape[0]
    return [np.array([np.count_nonzero(configs[:, p] == j) for j in range(d)], dtype=np.float64) / float(n) for p, d in enumerate(dims)]


def stat_defects(configs, cores, pair):
    """the worst |frequency - exact| / sigma, sigma = sqrt(p (1 - p) / n), over the one-site frequencies and over the
    joint table of the two sites of ``pair``; cells with p == 0 must have frequency 0"""
    n = configs.shape[0]
    P = dense_probs(cores)
    L = P.ndim
    worst1 = worst2 = 0.0

    def z(f, p):
        return np.abs(f - p) / np.sqrt(p * (1.0 - p) / n)

    for s in range(L):
        p = P.sum(axis=tuple(k for k in range(L) if k != s))
        f = histogram(configs, P.shape)[s]
        worst1 = max(worst1, z(f, p).max())
    a, b = pair
    p = P.sum(axis=tuple(k for k in range(L) if k not in pair))
    f = np.zeros_like(p)
    np.add.at(f, (configs[:, a], configs[:, b]), 1.0 / n)
    worst2 = z(f, p).max()
    return worst1, worst2
