"""tests/_biquad_i16_spec.py held to itself (the scalar and the numpy restatement agree bit for bit on adversarial inputs), to what the
project already trusts (oracle/spec.py: biquad_i32_df1 / _clamp, wherever no partial sum leaves i32 and no output leaves i16) and to
known answers.  CPU only."""
import math

import numpy as np
import pytest

from oracle import spec as O
from tests import _biquad_i16_spec as S

LP = [553, 1105, 553, 9363, -3382]  # from_sos(filter_lowpass(0.1), 13)


def _scalar_lanes(secs, state, x):
    """the scalar restatement on the numpy one's state layout: -> (y [frames, lanes], state after [4 n, lanes] uint32, Wraps)"""
    frames, lanes = x.shape
    n = len(secs)
    low = state.view(np.int32).astype(np.int16)
    y = np.empty((frames, lanes), np.int16)
    after = np.empty((4 * n, lanes), np.int32)
    w = S.Wraps()
    for lane in range(lanes):
        sts = [S.DirectForm1([int(low[4 * k, lane]), int(low[4 * k + 1, lane])], [int(low[4 * k + 2, lane]), int(low[4 * k + 3, lane])])
               for k in range(n)]
        y[:, lane] = S.chain(secs, sts, [int(v) for v in x[:, lane]], w)
        for k, st in enumerate(sts):
            after[4 * k:4 * k + 4, lane] = st.words()
    return y, after.view(np.uint32), w


@pytest.mark.parametrize("clamped", [False, True])
@pytest.mark.parametrize("n", [0, 1, 2, 4, 5, 9])
def test_restatements_agree(n, clamped):
    rng = np.random.default_rng(100 * n + clamped)
    wraps = S.Wraps()
    for trial in range(6):
        lanes, frames = int(rng.integers(1, 9)), int(rng.integers(1, 60))
        secs = S.random_sections(rng, n, clamped)
        x = S.inputs(rng, frames, lanes)
        st = S.random_state(rng, n, lanes) if trial else np.zeros((4 * n, lanes), np.uint32)
        ys, sts, w = _scalar_lanes(secs, st, x)
        stn = st.copy()
        yn = S.chain_np(secs, stn, x)
        assert np.array_equal(ys, yn), (n, clamped, trial, secs)
        assert np.array_equal(sts, stn), (n, clamped, trial, "state")
        wraps.i32 += w.i32
        wraps.i16 += w.i16
    if n:
        assert wraps.i32 and wraps.i16, "the inputs are meant to wrap"
    else:
        assert np.array_equal(ys, x)  # compose.rs:63-65


@pytest.mark.parametrize("frac", S.FRACS)
@pytest.mark.parametrize("coef", [S.I16_MAX, S.I16_MIN])
def test_extreme_coefficients_every_frac(frac, coef):
    """all-32767 and all--32768 coefficients, x from the edges of i16, a `u` that wraps the i16 sum and min > max"""
    rng = np.random.default_rng(frac + (coef & 7))
    x = S.inputs(rng, 40, 5)
    x[:4] = np.array(S.ADVERSARIAL, np.int16)[:, None]
    u_wraps = 0
    for secs in ([([coef] * 5, frac)], [([coef] * 5, frac, 32767, -100, 200)], [([coef] * 5, frac, -32768, 300, -300)],
                 [([coef] * 5, frac), ([-coef - 1] * 5, frac)]):
        st = S.random_state(rng, len(secs), 5)
        ys, sts, w = _scalar_lanes(secs, st, x)
        stn = st.copy()
        assert np.array_equal(ys, S.chain_np(secs, stn, x)) and np.array_equal(sts, stn), (secs,)
        if len(secs[0]) == 5:
            lo, hi = secs[0][3], secs[0][4]
            assert set(np.unique(ys)) <= ({lo, hi} | set(range(lo, hi + 1))), "clamp(v, min, max) yields min, max or a value between"
            u_wraps += w.i16
    assert u_wraps  # (F = 31 leaves y0 in {-1, 0}: only u = -32768 wraps there)


def test_pinned_by_the_i32_oracle():
    """Where no partial sum leaves i32 and no output leaves i16, Biquad<Q16<F>> IS oracle/spec.py: biquad_i32_df1 / _clamp with the same ba
    and F.  Low- and high-pass coefficients, f0 in 0.01..0.45, quantised to i16 at F in {10, 12, 13, 14}, 300 samples uniform in
    +-4000 and +-12000: 400 cases, none of which may have to be excluded for leaving range.
    The clamp form runs beside the plain one with u = 7.  A clamp that binds takes the recurrence off the linear filter's path, and
    what bounds y0 before the clamp then is |a1| B + |a2| B + (|b0| + |b1| + |b2|) A < 2.75 B + 3.76 A for these filters (B the limit, A
    the amplitude): at A = 4000 the limits are +-3000 (bound 23300, inside i16, and they bind all the time); at A = 12000 no limit
    keeps that bound inside i16, so the limits there are the whole of i16 and only u acts."""
    rng = np.random.default_rng(16)
    cases = excluded = compared = bound = 0
    for kind in (O.filter_lowpass, O.filter_highpass):
        for f0 in rng.uniform(0.01, 0.45, 25):
            for frac in (10, 12, 13, 14):
                for amp in (4000, 12000):
                    ba = S.from_sos(kind(float(f0)), frac)
                    assert ba == [max(S.I16_MIN, min(S.I16_MAX, v)) for v in O.biquad_i32_from_sos(kind(float(f0)), frac)]
                    xs = [int(v) for v in rng.integers(-amp, amp + 1, 300)]
                    w, st = S.Wraps(), S.DirectForm1()
                    ys = [S.df1(ba, frac, st, v, w) for v in xs]
                    wc, stc = S.Wraps(), S.DirectForm1()
                    lo, hi = (-3000, 3000) if amp == 4000 else (S.I16_MIN, S.I16_MAX)
                    yc = [S.df1_clamp(ba, frac, 7, lo, hi, stc, v, wc) for v in xs]
                    bound += amp == 4000 and (lo in yc or hi in yc)
                    cases += 1
                    if w.i32 or w.i16 or wc.i32 or wc.i16:
                        excluded += 1
                        continue
                    so, soc = O.DirectForm1(), O.DirectForm1()
                    assert ys == [O.biquad_i32_df1(ba, frac, so, v) for v in xs], (kind.__name__, f0, frac, amp)
                    assert yc == [O.biquad_i32_df1_clamp(ba, frac, 7, lo, hi, soc, v) for v in xs], (kind.__name__, f0, frac, amp)
                    assert st.words() == [so.x[0], so.x[1], so.y[0], so.y[1]] and stc.words() == [soc.x[0], soc.x[1], soc.y[0], soc.y[1]]
                    compared += len(xs)
    assert cases == 400 and excluded == 0, (cases, excluded)
    assert compared == 400 * 300 and bound > 100


KNOWN = [
    (LP, 13, [1000, -2000, 32767, -32768, 0, 0, 5, 12345], [67, 76, 2068, 4405, 1972, -1777, -2845, -1685], None),
    ([32767] * 5, 0, [32767, 32767, -32768, 1, 2], [1, -32767, 0, -1, 32766], [2, 1, 32766, -1]),  # the wrapping case
]


@pytest.mark.parametrize("ba,frac,x,y,state", KNOWN)
def test_known_answers(ba, frac, x, y, state):
    st = S.DirectForm1()
    assert [S.df1(ba, frac, st, v) for v in x] == y
    if state is not None:
        assert st.words() == state
    stn = np.zeros((4, 1), np.uint32)
    assert S.chain_np([(ba, frac)], stn, np.array(x, np.int16)[:, None])[:, 0].tolist() == y
    assert stn.view(np.int32)[:, 0].tolist() == st.words()


def test_known_coefficients():
    assert S.from_sos(O.filter_lowpass(0.1), 13) == LP
    assert S.from_sos_np([O.filter_lowpass(0.1)], 13)[0].tolist() == LP


@pytest.mark.parametrize("frac", range(0, 15))
def test_identity(frac):
    """ba = [1 << F, 0, 0, 0, 0]: y = x for any x (F <= 14 keeps 1 << F inside i16)"""
    rng = np.random.default_rng(frac)
    x = S.inputs(rng, 50, 3)
    st = S.random_state(rng, 1, 3)
    assert np.array_equal(S.chain_np([([1 << frac, 0, 0, 0, 0], frac)], st.copy(), x), x)
    assert np.array_equal(_scalar_lanes([([1 << frac, 0, 0, 0, 0], frac)], st, x)[0], x)


def test_from_sos_restatements_agree():
    rng = np.random.default_rng(5)
    sos = S.sos_rows(rng, 2000)
    seen = set()
    for frac in (0, 13, 15, 31):
        got = S.from_sos_np(sos, frac)
        for row, g in zip(sos, got):
            with np.errstate(all="ignore"):
                want = S.from_sos([float(v) for v in row], frac) if row[3] != 0.0 else None
            if want is None:  # 1.0 / 0.0 raises in Python: the C double gives inf, products with it +-inf or NaN
                a0 = math.inf
                want = []
                for v in (row[0] * a0, row[1] * a0, row[2] * a0, -row[4] * a0, -row[5] * a0):
                    want.append(0 if math.isnan(v) else (S.I16_MAX if v > 0 else S.I16_MIN))
            assert g.tolist() == want, (row, frac)
            seen |= set(want)
    assert {S.I16_MAX, S.I16_MIN, 0} <= seen
    assert S.from_sos([0.5 / 8192, -0.5 / 8192, 1.5 / 8192, 1.0, 2.5 / 8192, -2.5 / 8192], 13) == [1, -1, 2, -3, 3]  # half away from zero
