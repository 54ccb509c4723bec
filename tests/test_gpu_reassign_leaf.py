"""GPU: the two kernels of csrc/vq_reassign.hip (ops.vq_reassign_plan / vq_reassign_apply, mcquic_amd.CodebookReassign) against BOTH
yardsticks -- the numpy restatement tests/_reassign_ref.py and the eager torch method on CPU (pinned to each other in
tests/test_reassign_ref.py) -- bit for bit: the new codebook, `source` and the `changed` mask; any differing element fails.

The inputs (`_reassign_ref.regime_case`) make the yardsticks exact: frequencies are multiples of 2^-20 with row sums below 16 (exact in
any order), codewords are integers / 8 (a squared distance is 0 or >= 1/64, far from 1e-4).  Several group regimes share one launch."""
import numpy as np
import pytest
import torch

import _reassign_ref as RR
from test_reassign_ref import torch_reassign

pytestmark = pytest.mark.gpu


def _state(dev, seed=0, count=0):
    """A record whose next step fires with every=1."""
    from mcquic_amd import ops
    words = [0] * ops.REASSIGN_STATE_WORDS
    words[0] = words[1] = count
    words[5] = seed
    return torch.tensor(words, dtype=torch.int64).to(dev)


def _run(dev, cases, priorities=True, state=None, every=1):
    """One plan + apply over `cases` = [(codebook, raw_freq, priority)] as one multi-level launch; host copies of what it left."""
    from mcquic_amd import ops
    state = _state(dev) if state is None else state
    cbs = [torch.from_numpy(c).to(dev) for c, _, _ in cases]
    freqs = [torch.from_numpy(f).to(dev) for _, f, _ in cases]
    prios = [torch.from_numpy(p).to(dev) for _, _, p in cases] if priorities else None
    source, refill = ops.vq_reassign_plan(freqs, state, every, priorities=prios)
    changed = ops.vq_reassign_apply(cbs, source, refill, state, every)
    torch.cuda.synchronize()
    return [c.cpu().numpy() for c in cbs], [s.cpu().numpy() for s in source], [c.cpu().numpy() for c in changed], state.cpu()


def _assert_level(case, new, source, changed):
    cb, raw, prio = case
    want_new, want_source, want_changed = RR.reassign(cb, raw, prio)
    t_new, t_changed = torch_reassign(cb, raw, prio)
    assert source.dtype == np.int32
    np.testing.assert_array_equal(source, want_source)
    for w_new, w_changed in ((want_new, want_changed), (t_new, t_changed)):
        assert np.array_equal(new.view(np.uint32), w_new.view(np.uint32)), f"{int((new.view(np.uint32) != w_new.view(np.uint32)).sum())} elements differ"
        np.testing.assert_array_equal(changed, w_changed)
    return int(want_changed.sum())


# (m, k, d, regimes, ties): m = 1 shapes take the regime that exercises most; the 6-group cases hold every regime in one launch
SHAPES = [(1, 2, 1, ("half",), False), (2, 5, 3, ("half+1", "all-but-one"), False), (3, 64, 16, ("one", "half+1", "all"), False),
          (6, 64, 16, RR.REGIMES, False), (6, 64, 16, RR.REGIMES, True), (6, 33, 4, RR.REGIMES, True),
          (2, 4096, 8, ("half", "all-but-one"), False), (1, 8192, 64, ("half+1",), False), (1, 8192, 1, ("all-but-one",), True)]


@pytest.mark.parametrize("m,k,d,regimes,ties", SHAPES)
def test_one_level_equals_both_yardsticks_bit_for_bit(dev, m, k, d, regimes, ties):
    case = RR.regime_case(m, k, d, seed=m * 1000 + k + d, regimes=regimes, ties=ties)
    new, source, changed, state = _run(dev, [case])
    moved = _assert_level(case, new[0], source[0], changed[0])
    assert int(state[0]) == 1 and int(state[1]) == 1 and int(state[2]) == 1 and int(state[3]) == moved
    assert float(state.view(torch.float32)[8]) == float(np.float32(moved) / np.float32(m * k))


def test_three_levels_in_one_launch(dev):
    """The level table: k = 8192 / 2048 / 512 with m = 2, the shapes of the qp = 2 model, every level in its own regimes."""
    cases = [RR.regime_case(2, k, 8, seed=k, regimes=regimes) for k, regimes in ((8192, ("half+1", "one")), (2048, ("all-but-one", "none")),
                                                                                  (512, ("all", "half")))]
    new, source, changed, state = _run(dev, cases)
    moved = sum(_assert_level(c, n, s, ch) for c, n, s, ch in zip(cases, new, source, changed))
    assert int(state[3]) == moved and int(state[2]) == 1
    assert float(state.view(torch.float32)[8]) == float(np.float32(moved) / np.float32(2 * (8192 + 2048 + 512)))


def test_more_levels_than_one_table_holds(dev):
    """The chunking: more levels than mcq_vq_max_levels() at k = 4 -- one count, one firing step, `moved` summed over the chunks."""
    from mcquic_amd import _lib
    levels = int(_lib.load().mcq_vq_max_levels()) + 3
    cases = [RR.regime_case(2, 4, 2, seed=l, regimes=RR.REGIMES[1 + l % 4:]) for l in range(levels)]
    new, source, changed, state = _run(dev, cases)
    moved = sum(_assert_level(c, n, s, ch) for c, n, s, ch in zip(cases, new, source, changed))
    assert moved > 0 and int(state[3]) == moved
    assert [int(v) for v in state[:3]] == [1, 1, 1] and int(state[6]) == levels


def test_drawn_priorities_are_hash_uniform_of_the_snapshot(dev):
    """Without caller priorities level l draws ops.hash_uniform({seed, offset + l}, REASSIGN_STREAM, (m, k)); the offset advances by the
    level count, and only on a firing step."""
    from mcquic_amd import ops
    shapes = [(3, 64, 4), (2, 33, 2)]
    regimes = ("half+1", "all-but-one", "half+1")                     # crowded groups: the priorities decide who is refilled
    cases = [RR.regime_case(m, k, d, seed=7 + k, regimes=regimes) for m, k, d in shapes]
    state = _state(dev, seed=1234)
    state[6] = 40
    snaps = [torch.tensor([1234, 40 + l], dtype=torch.int64).to(dev) for l in range(2)]
    drawn = [ops.hash_uniform(s, ops.REASSIGN_STREAM, (m, k)).cpu().numpy() for s, (m, k, _) in zip(snaps, shapes)]
    assert not np.array_equal(drawn[0][:2, :33], drawn[1])            # (the levels draw under their own offsets)
    new, source, changed, after = _run(dev, cases, priorities=False, state=state, every=2)       # count 0 -> 1: (1 + 1) % 2 == 0 fires
    for (cb, raw, _), p, n, s, ch in zip(cases, drawn, new, source, changed):
        _assert_level((cb, raw, p), n, s, ch)
    assert int(after[6]) == 42 and int(after[2]) == 1
    new2, _, _, after2 = _run(dev, cases, priorities=False, state=after.to(dev), every=2)         # count 1 -> 2: does not fire
    assert int(after2[6]) == 42 and int(after2[0]) == 2 and int(after2[2]) == 1
    assert all(np.array_equal(n, c[0]) for n, c in zip(new2, cases))


def _model(dev, seed=0):
    from mcquic_amd import Compressor
    torch.manual_seed(seed)
    model = Compressor(16, 2, [64, 32, 16]).to(dev)
    with torch.no_grad():
        for lv, f in enumerate(model._quantizer._entropyCoder._freqEMA):
            case = RR.regime_case(2, f.shape[1], 1, seed=lv, regimes=("half+1", "one"))
            f.copy_(torch.from_numpy(case[1]).to(dev))
    return model


def _expected(model, snapshot):
    """The numpy yardstick on the model's current codebooks and frequencies, priorities from `snapshot` = (seed, offset)."""
    from mcquic_amd import ops
    out = []
    for lv, (enc, f) in enumerate(zip(model._quantizer._encoders, model._quantizer._entropyCoder._freqEMA)):
        snap = torch.tensor([snapshot[0], snapshot[1] + lv], dtype=torch.int64).to(f.device)
        prio = ops.hash_uniform(snap, ops.REASSIGN_STREAM, tuple(f.shape)).cpu().numpy()
        out.append(RR.reassign(enc.Codebook.detach().cpu().numpy(), f.detach().cpu().numpy(), prio))
    return out


def test_decision_words_every_three_over_seven_calls(dev):
    """every=3: the step fires when the completed count s after the update has (s + 1) % 3 == 0 -- calls 2 and 5, not call 7 (s + 1 = 8);
    on every other call not one codebook byte changes."""
    import mcquic_amd
    model = _model(dev)
    re = mcquic_amd.CodebookReassign(model, freq=3, seed=5)
    fired_on = []
    for call in range(1, 8):
        before = [c.detach().clone() for c in model.Codebooks]
        want = _expected(model, (5, 3 * len(fired_on)))
        re.step()
        same = all(torch.equal(a, b.detach()) for a, b in zip(before, model.Codebooks))
        if call in (2, 5):
            assert not same
            for (new, _, changed), cb, ch in zip(want, model.Codebooks, re.changed):
                assert np.array_equal(cb.detach().cpu().numpy().view(np.uint32), new.view(np.uint32))
                np.testing.assert_array_equal(ch.cpu().numpy(), changed)
            fired_on.append(call)
            with torch.no_grad():                                     # fresh codewords for the next firing step to move
                for cb in model.Codebooks:
                    cb.copy_(torch.randint(-64, 65, cb.shape, device=dev).float() / 8)
        else:
            assert same, call
        assert int(re.count) == call
    out = re.read()
    assert fired_on == [2, 5] and out["fired"] == 2 and out["count"] == 7 and out["offset"] == 6
    assert 0.0 < out["Stat/ReAssignProportion"] < 1.0 and out["moved"] > 0


def test_a_set_skip_flag_on_a_firing_call_moves_nothing(dev):
    import mcquic_amd
    model = _model(dev)
    re = mcquic_amd.CodebookReassign(model, freq=1, seed=9)
    flag = torch.ones(1, dtype=torch.int32, device=dev)
    before = [c.detach().clone() for c in model.Codebooks]
    state = re._state.clone()
    re.step(skip=flag)
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, model.Codebooks))
    assert torch.equal(state, re._state)                               # count, generator state and scalars
    flag.zero_()
    want = _expected(model, (9, 0))
    re.step(skip=flag)                                                 # the next clean call fires as if the void one had not happened
    assert int(re.count) == 1 and int(re.fired) == 1
    for (new, _, _), cb in zip(want, model.Codebooks):
        assert np.array_equal(cb.detach().cpu().numpy().view(np.uint32), new.view(np.uint32))


def test_state_dict_resumes_on_the_same_step_with_the_same_bits(dev):
    import mcquic_amd
    a, b = _model(dev, seed=1), _model(dev, seed=1)
    ra = mcquic_amd.CodebookReassign(a, freq=4, seed=77)
    for _ in range(5):                                                 # fires on call 3; offset moves on
        ra.step()
    rb = mcquic_amd.CodebookReassign(b, freq=4, seed=0)
    rb.load_state_dict(ra.state_dict())
    with torch.no_grad():
        for ca, cb in zip(a.Codebooks, b.Codebooks):
            cb.copy_(ca)
    assert rb.read() == ra.read() and ra.read()["fired"] == 1
    for call in range(6, 9):
        before = [c.detach().clone() for c in b.Codebooks]
        ra.step()
        rb.step()
        assert all(torch.equal(x.detach(), y.detach()) for x, y in zip(a.Codebooks, b.Codebooks))
        assert all(torch.equal(x, y.detach()) for x, y in zip(before, b.Codebooks)) == (call != 7)
    assert rb.read() == ra.read() and rb.read()["fired"] == 2
    with pytest.raises(ValueError, match="freq"):
        mcquic_amd.CodebookReassign(b, freq=5).load_state_dict(ra.state_dict())


def test_refusals(dev):
    """A non-contiguous codebook, a row longer than the plan kernel's LDS arrays (at both layers), and a model without per-level pairs."""
    import mcquic_amd
    from mcquic_amd import _lib, ops
    case = RR.regime_case(2, 8, 4, seed=0)
    state = _state(dev)
    freq = torch.from_numpy(case[1]).to(dev)
    source, refill = ops.vq_reassign_plan([freq], state, 1)
    wide = torch.zeros((2, 8, 8), device=dev)[:, :, ::2]
    with pytest.raises(ValueError, match="contiguous"):
        ops.vq_reassign_apply([wide], source, refill, state, 1)
    with pytest.raises(ValueError, match="contiguous"):
        ops.vq_reassign_plan([freq], torch.zeros(14, dtype=torch.int64, device=dev)[::2], 1)
    kmax = int(_lib.load().mcq_vq_reassign_max_k())
    assert kmax == 8192
    big = torch.ones((1, kmax + 1), device=dev)
    with pytest.raises(ValueError, match="LDS"):
        ops.vq_reassign_plan([big], state, 1)
    lib = _lib.load()
    import ctypes
    one = (ctypes.c_int32 * 1)
    ptr = (ctypes.c_void_p * 1)
    assert lib.mcq_vq_reassign_plan(ptr(big.data_ptr()), None, one(1), one(kmax + 1), 1, 0, 1, ptr(big.data_ptr()), ptr(big.data_ptr()),
                                    state.data_ptr(), 1, 0, None, None) == _lib.MCQ_EINVAL
    with pytest.raises(NotImplementedError, match="ResidualBackwardQuantizer"):
        mcquic_amd.CodebookReassign(mcquic_amd.Neon(32, 256, [8, 4, 2, 2]), freq=10)
    with pytest.raises(ValueError, match="freq"):
        mcquic_amd.CodebookReassign(_model(dev), freq=0)
