"""numpy float64 restatement of csrc/vq_kmeans.hip: sequential accumulation in ascending vector order, the centroid update with
its inertia and skip rules, and the seeding pick rule with the uniforms as input.  Layouts are mcq_vq_assign_f32's."""
import numpy as np


def vectors(x, m):
    """[N, m*d, h, w] -> float64 [m, V, d], vector index v = (n, y, x) ascending."""
    N, c, h, w = x.shape
    d = c // m
    return np.asarray(x, np.float64).reshape(N, m, d, h * w).transpose(1, 0, 3, 2).reshape(m, N * h * w, d)


def code_rows(codes):
    """[N, m, h, w] -> int64 [m, V]."""
    N, m, h, w = codes.shape
    return np.asarray(codes, np.int64).reshape(N, m, h * w).transpose(1, 0, 2).reshape(m, N * h * w)


def new_acc(m, k, d):
    return np.zeros((m, k, d), np.float64), np.zeros((m, k), np.float64), np.zeros((m, k), np.int64)


def accumulate(x, codes, acc):
    """One batch onto acc = (sums, sqsums, counts), vector by vector; a code outside [0, k) is skipped."""
    sums, sqsums, counts = acc
    m, k, d = sums.shape
    xv, cv = vectors(x, m), code_rows(codes)
    for g in range(m):
        for v in range(xv.shape[1]):
            c = int(cv[g, v])
            if 0 <= c < k:
                sums[g, c] += xv[g, v]
                sqsums[g, c] += float((xv[g, v] * xv[g, v]).sum())
                counts[g, c] += 1
    return acc


def update(codebook, acc):
    """-> (new codebook float32, inertia float64 [m] against the OLD codewords, empty int64 [m])."""
    sums, sqsums, counts = acc
    old = np.asarray(codebook, np.float32)
    new = old.copy()
    m, k, d = old.shape
    inertia, empty = np.zeros(m, np.float64), np.zeros(m, np.int64)
    for g in range(m):
        for c in range(k):
            co = old[g, c].astype(np.float64)
            inertia[g] += sqsums[g, c] - 2.0 * float((co * sums[g, c]).sum()) + counts[g, c] * float((co * co).sum())
            if counts[g, c] > 0:
                new[g, c] = (sums[g, c] / counts[g, c]).astype(np.float32)
            else:
                empty[g] += 1
    return new, inertia, empty


def picks(u, V):
    """Vector number per draw: min(V - 1, floor(u V)), the product in float64 (exact: u = i / 2^24)."""
    return np.minimum(V - 1, np.floor(np.asarray(u, np.float64) * V).astype(np.int64))


def seed(x, codebook, u, counts=None):
    """codebook[g, c] = vector picks(u[g, c]) of group g -- everywhere (counts None) or where counts[g, c] == 0."""
    old = np.asarray(codebook, np.float32)
    m, k, d = old.shape
    xv = vectors(x, m)
    p = picks(np.asarray(u).reshape(m, k), xv.shape[1])
    new = old.copy()
    for g in range(m):
        for c in range(k):
            if counts is None or counts[g, c] == 0:
                new[g, c] = xv[g, p[g, c]].astype(np.float32)
    return new
