"""tests/_biquad_i16_bylane_spec.py against the specification the project already trusts (tests/_biquad_i16_spec.py): for every lane l,
column l of the by-lane result equals `S.chain_np` run on column l alone with lane l's sections and state, and the scalar `S.chain`, which
counts the wraps.  No GPU, no library."""
import numpy as np
import pytest

from tests import _biquad_i16_bylane_spec as B
from tests import _biquad_i16_spec as S

LANES, FRAMES = 7, 40


def _scalar_states(st, n, lane):
    words = st.view(np.int32).reshape(4 * n, -1)[:, lane].astype(np.int16)
    return [S.DirectForm1(x=(int(words[4 * k]), int(words[4 * k + 1])), y=(int(words[4 * k + 2]), int(words[4 * k + 3]))) for k in range(n)]


def _check_lanes(lane_secs, frac, coef, st, x):
    """the by-lane chain, then each lane alone on both forms of the shared specification"""
    n = coef.shape[0]
    got_st = st.copy()
    got = B.chain_np(coef, frac, got_st, x)
    wraps = S.Wraps()
    for l, secs in enumerate(lane_secs):
        assert secs == B.sections_of(coef, frac, l)
        one_st = np.ascontiguousarray(st[:, l:l + 1])
        want = S.chain_np(secs, one_st, np.ascontiguousarray(x[:, l:l + 1]))
        assert np.array_equal(got[:, l:l + 1], want), l
        assert np.array_equal(got_st[:, l:l + 1], one_st), (l, "state")
        states = _scalar_states(st, n, l)
        assert S.chain(secs, states, [int(v) for v in x[:, l]], wraps) == got[:, l].tolist(), (l, "scalar")
        words = np.array([w for s in states for w in s.words()], np.int32)
        assert np.array_equal(got_st[:, l].view(np.int32), words), (l, "scalar state")  # sign-extended
    return wraps


@pytest.mark.parametrize("clamped", [False, True])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_every_lane_equals_the_shared_specification(n, clamped):
    total = S.Wraps()
    for seed in range(4):
        rng = np.random.default_rng(100 * n + 10 * clamped + seed)
        lane_secs, frac, coef = B.random_bank(rng, n, clamped, LANES)
        w = _check_lanes(lane_secs, frac, coef, S.random_state(rng, n, LANES), S.inputs(rng, FRAMES, LANES))
        total.i32 += w.i32
        total.i16 += w.i16
    assert total.i32 > 0 and total.i16 > 0  # the wild sections do leave i32 and i16: the wrapping is exercised, not avoided


@pytest.mark.parametrize("clamped", [False, True])
@pytest.mark.parametrize("frac", [0, 13, 15, 16, 31])
def test_sections_at_the_edges_of_i16(frac, clamped):
    """lanes whose sections are all 32767 and all -32768, beside random ones, at several F"""
    rng = np.random.default_rng(frac + 50 * clamped)
    lane_secs, _, _ = B.random_bank(rng, 2, clamped, LANES, frac)
    for l, v in ((0, S.I16_MAX), (3, S.I16_MIN), (6, S.I16_MAX)):
        lane_secs[l] = [([v] * 5, frac, *sec[2:]) for sec in lane_secs[l]]
    lane_secs[6][1] = ([S.I16_MIN] * 5, frac, *lane_secs[6][1][2:])  # both in one lane
    coef = B.planes(lane_secs, clamped)
    _check_lanes(lane_secs, frac, coef, S.random_state(rng, 2, LANES), S.inputs(rng, FRAMES, LANES))


def test_equal_lanes_equal_the_shared_chain():
    """a bank whose lanes all hold the same sections is the shared-coefficient chain"""
    rng = np.random.default_rng(9)
    for clamped in (False, True):
        secs = [(s[0], 14, *s[2:]) for s in S.random_sections(rng, 3, clamped)]
        st, x = S.random_state(rng, 3, LANES), S.inputs(rng, FRAMES, LANES)
        a_st, b_st = st.copy(), st.copy()
        a = B.chain_np(B.planes([secs] * LANES, clamped), 14, a_st, x)
        b = S.chain_np(secs, b_st, x)
        assert np.array_equal(a, b) and np.array_equal(a_st, b_st)


def test_planes_layout_and_no_sections():
    rng = np.random.default_rng(1)
    lane_secs, frac, coef = B.random_bank(rng, 2, True, 3)
    assert coef.shape == (2, 8, 3) and coef.dtype == np.int16
    flat = coef.reshape(-1)
    for l in range(3):
        for k in range(2):
            vals = list(lane_secs[l][k][0]) + list(lane_secs[l][k][2:])
            assert [int(flat[(k * 8 + v) * 3 + l]) for v in range(8)] == vals  # coef[(k*CV + v)*lanes + l]
    frac2, big = B.random_planes(rng, 3, False, 1000)
    assert big.shape == (3, 5, 1000) and 0 <= frac2 <= 31
    assert (big == S.I16_MAX).all(axis=1).any() and (big == S.I16_MIN).all(axis=1).any()
    x, st = S.inputs(rng, 5, 3), S.random_state(rng, 1, 3)
    assert np.array_equal(B.chain_np(np.zeros((0, 5, 3), np.int16), 0, np.zeros((0, 3), np.uint32), x), x)  # n == 0 copies
    assert st.shape == (4, 3)
