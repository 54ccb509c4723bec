"""An independent numpy restatement of the codebook-reassignment rule (mcquic_amd/modules/quantizer.py `reAssignCodebook`, the reference's
mcquic/modules/quantizer.py:111-136): `np.lexsort` for the two stable orders, the row sum in double rounded once to float32.  No torch,
no kernel: the second yardstick of csrc/vq_reassign.hip beside the eager torch method (tests/test_reassign_ref.py pins one to the other)."""
import numpy as np

EPS = np.float32(1e-6)


def normalised(raw_freq):
    """f / s per row, s = the row's sum in double rounded once to float32."""
    raw = np.asarray(raw_freq, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = raw.astype(np.float64).sum(-1, keepdims=True).astype(np.float32)      # (a sum past float32's range is inf: every f / s is 0)
        return raw / s


REGIMES = ("none", "one", "half", "half+1", "all-but-one", "all")


def regime_case(m, k, d, seed, regimes=REGIMES, ties=False):
    """Inputs on which every yardstick is exact.  Frequencies are multiples of 2^-20 with a row sum below 16, so the sum is exact in any
    order and any precision; codewords are integers / 8, so a squared distance is 0 or >= 1/64, far from 1e-4.  Group g takes
    regimes[g % len(regimes)], by its number of dead codewords: none, one, exactly k // 2, k // 2 + 1 (the first crowded case), all but
    one (the donors past the live one are refilled rows themselves: the read-before-write case), all.  A dead entry is 0 or 2^-20 of a
    row sum in [4, 8); a live one at least 32 * 2^-20.  "all" cannot be reached with a finite sum (k entries below 1e-6 do not add up
    to 1): its row is 2^127 throughout, whose sum is inf in float32, so every f / s is 0.  Where a group has dead codewords, index 0 is
    dead, and from two on index k - 1.  `ties`: equal frequencies among the live and equal priorities among the dead ones.
    Returns (codebook [m, k, d], raw_freq [m, k], priority [m, k]) as float32 numpy arrays."""
    rng = np.random.default_rng(seed)
    cb = rng.integers(-64, 65, size=(m, k, d)).astype(np.float32) / 8
    raw = np.zeros((m, k), dtype=np.float32)
    prio = np.zeros((m, k), dtype=np.float32)
    unit = np.float32(2.0 ** -20)
    for g in range(m):
        regime = regimes[g % len(regimes)]
        ndead = {"none": 0, "one": 1, "half": k // 2, "half+1": k // 2 + 1, "all-but-one": k - 1, "all": k}[regime]
        ndead = min(ndead, k if regime == "all" else k - 1)                  # (a finite row needs a live codeword)
        prio[g] = rng.integers(0, 3 if ties else 1 << 20, size=k).astype(np.float32) / np.float32(1 << 20)
        if regime == "all":
            raw[g] = np.float32(2.0 ** 127)
            continue
        dead = np.zeros(k, dtype=bool)
        dead[:1] = ndead >= 1
        dead[k - 1:] = ndead >= 2
        rest = np.nonzero(~dead)[0]
        dead[rng.permutation(rest)[: ndead - int(dead.sum())]] = True
        nlive = k - ndead
        hi = (8 << 20) // nlive
        lo = hi // 2
        assert lo >= 32
        units = rng.integers(lo, lo + 3 if ties else hi, size=k)
        raw[g] = np.where(dead, rng.integers(0, 2, size=k), units).astype(np.float32) * unit
    return cb, raw, prio


def plan(raw_freq, priority):
    """(source int32 [m, k], refill bool [m, k]): the donor index per codeword (its own where nothing moves)."""
    fn = normalised(raw_freq)
    prio = np.asarray(priority, dtype=np.float32)
    m, k = fn.shape
    half = k // 2
    index = np.arange(k)
    source = np.tile(index.astype(np.int32), (m, 1))
    refill = np.zeros((m, k), dtype=bool)
    for g in range(m):
        dead = fn[g] < EPS
        lineup = np.lexsort((index, np.where(dead, prio[g], np.float32(np.inf))))         # ascending key, ties by index
        place = np.empty(k, dtype=np.int64)
        place[lineup] = index
        refill[g] = dead & (place < half)
        crowded = int(dead.sum()) > half
        score = np.where(dead & crowded, np.where(refill[g], np.float32(0), np.float32(-1)), fn[g]).astype(np.float32)
        donors = np.lexsort((index, -score))                                              # descending score, ties by index
        slots = np.nonzero(refill[g])[0]                                                  # the refilled codewords in index order
        source[g, slots] = donors[: len(slots)]
    return source, refill


def reassign(codebook, raw_freq, priority):
    """(new_codebook float32 [m, k, d], source int32 [m, k], changed bool [m, k]); every donor row is read from the OLD codebook."""
    old = np.asarray(codebook, dtype=np.float32)
    source, refill = plan(raw_freq, priority)
    new = old.copy()
    for g in range(old.shape[0]):
        new[g, refill[g]] = old[g, source[g, refill[g]]]
    diff = new - old
    dist = np.zeros(old.shape[:2], dtype=np.float32)
    for j in range(old.shape[2]):                                                         # float32, summed over d in index order
        dist = dist + diff[..., j] * diff[..., j]
    return new, source, dist > np.float32(1e-4)
