"""The reference side of the float special-value cases, kept honest without a GPU: for every case of the shared tables
(tests/_float_special.py) the CPU oracle is compared, under `assert_same_float`, with an independent per-sample restatement
in numpy float32 / float64 — one rounded operation per reference operation, left to right, the clamp written as its two
comparisons — and must meet the conditions that make a comparison against it worth something: the NaN cap, NaN / inf / normal
control lanes present per case, subnormal / +0 / -0 present per entry.

The restatement is elementwise over the lanes of a frame (numpy's float32 / float64 multiply and add are the IEEE
operations, one rounding each), sequential over frames; the big lane counts are restated on their first 64 lanes, the
conditions always see the full oracle output.  Reference lines restated: src/iir/biquad.rs:339-383,418-440,
src/iir/normal.rs:37-58, src/hbf.rs:46-68,70-138,163-185,207-227, src/lockin.rs:17-27."""
import time

import numpy as np
import pytest

from tests import _float_special as S

RESTATE_LANES = 64


def clamp(v, lo, hi):
    """num_traits::clamp: `if v < lo { lo } else if v > hi { hi } else { v }` — a NaN v fails both comparisons."""
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


class Coef:
    """Section k's coefficients as scalars of the sample type (shared sections) or per-lane arrays (`_bylane`)."""

    def __init__(self, case, inp, lanes):
        self.F = case.dtype
        self.rows, self.coef, self.cl = inp.rows, (None if inp.coef is None else inp.coef[:, :, lanes]), inp.clamp

    def ba(self, k):
        return [self.F(v) for v in self.rows[k]] if self.coef is None else [self.coef[k, v] for v in range(5)]

    def clamp(self, k):
        return [self.F(v) for v in self.cl] if self.coef is None else [self.coef[k, v] for v in (5, 6, 7)]


def df1_section(ba, cl, s, x):
    """biquad.rs:366-383 (and the clamped impl next to it): s = [x1, x2, y1, y2] rows; x, result [frames, lanes]."""
    b0, b1, b2, a1, a2 = ba
    y = np.empty_like(x)
    x1, x2, y1, y2 = s
    for f in range(x.shape[0]):
        x0 = x[f]
        acc = b0 * x0
        acc = acc + b1 * x1
        acc = acc + b2 * x2
        acc = acc + a1 * y1
        acc = acc + a2 * y2
        if cl is not None:
            acc = clamp(acc + cl[0], cl[1], cl[2])
        x2, x1, y2, y1 = x1, x0, y1, acc
        y[f] = acc
    s[:] = [x1, x2, y1, y2]
    return y


def df2t_section(ba, cl, s, x):
    """biquad.rs:418-428 and :430-440: s = [s0, s1]."""
    b0, b1, b2, a1, a2 = ba
    y = np.empty_like(x)
    s0, s1 = s
    for f in range(x.shape[0]):
        x0 = x[f]
        y0 = s0 + b0 * x0
        if cl is not None:
            y0 = clamp(y0 + cl[0], cl[1], cl[2])
        s0 = (s1 + b1 * x0) + a1 * y0
        s1 = b2 * x0 + a2 * y0
        y[f] = y0
    s[:] = [s0, s1]
    return y


def normal_section(ba, s, x):
    """normal.rs:37-58: ba = [b0, b1, b2, p.re, p.im], s = [x1, x2, y0 (in phase), y1 (quadrature)]."""
    b0, b1, b2, re, im = ba
    y = np.empty_like(x)
    x1, x2, y0o, y1o = s
    for f in range(x.shape[0]):
        x0 = x[f]
        acc = b0 * x0
        acc = acc + b1 * x1
        acc = acc + b2 * x2
        acc = acc + re * y1o
        acc = acc + (-im) * y0o
        y0 = im * y1o + re * y0o
        x2, x1, y0o, y1o = x1, x0, y0, acc
        y[f] = y0
    s[:] = [x1, x2, y0o, y1o]
    return y


def cascade(co, n, s, x):
    """biquad.rs:339-364: sample-major fold; section k's input history is section k-1's output history.
    s = [x0, x1, (y0, y1) x n]."""
    y = np.empty_like(x)
    h = [s[i] for i in range(2 + 2 * n)]
    bas = [co.ba(k) for k in range(n)]
    for f in range(x.shape[0]):
        x0, xi = x[f], 0
        for k in range(n):
            b0, b1, b2, a1, a2 = bas[k]
            yi = 2 + 2 * k
            acc = b0 * x0
            acc = acc + b1 * h[xi]
            acc = acc + b2 * h[xi + 1]
            acc = acc + a1 * h[yi]
            acc = acc + a2 * h[yi + 1]
            h[xi + 1], h[xi] = h[xi], x0
            x0, xi = acc, yi
        h[xi + 1], h[xi] = h[xi], x0
        y[f] = x0
    s[:] = h
    return y


def restate_iir(case, inp, x, lo, sv, lanes):
    """x [frames, L, 1] -> y [frames, L, rout]; sv [values, L] float state values, updated."""
    co, n, form = Coef(case, inp, lanes), case.n, case.form
    s = [sv[i] for i in range(sv.shape[0])]
    if form == "cascade":
        y = cascade(co, n, s, x[:, :, 0])[:, :, None]
    elif form == "lockin":  # lockin.rs:17-27 with `Biquad<f32>` arms: arm q filters x * lo[q]; state I: n x 4, then Q: n x 4
        y = np.empty(x.shape[:2] + (2,), x.dtype)
        for q in range(2):
            v = x[:, :, 0] * lo[:, :, q]
            for k in range(n):
                i = (q * n + k) * 4
                sk = s[i:i + 4]
                v = df1_section(co.ba(k), None, sk, v)
                s[i:i + 4] = sk
            y[:, :, q] = v
    else:  # `[C] x [S]`: every section over its own state record
        vals = {"df1": 4, "df2t": 2, "normal": 4}[form]
        v = x[:, :, 0]
        for k in range(n):
            sk = s[k * vals:(k + 1) * vals]
            cl = co.clamp(k) if case.clamp else None
            v = normal_section(co.ba(k), sk, v) if form == "normal" else (df1_section if form == "df1" else df2t_section)(co.ba(k), cl, sk, v)
            s[k * vals:(k + 1) * vals] = sk
        y = v[:, :, None]
    sv[:] = np.stack(s)
    return y


def get(taps, w, n, span, sym=True):
    """hbf.rs:46-68 over n windows of `span` samples starting at w[i]: `sum` is a sequential fold seeded with -0.0."""
    acc = np.full((n,) + w.shape[1:], -0.0, w.dtype)
    for k in range(len(taps)):
        nw, od = w[span - 1 - k:span - 1 - k + n], w[k:k + n]
        acc = acc + ((nw + od) if sym else (nw - od)) * taps[k]
    return acc


def restate_fir(case, inp, x, sv):
    """hbf.rs:70-138; sv = the last 2M - 1 + odd inputs, oldest first."""
    kind, m = case.fir
    odd, sym = kind in (0, 2), kind in (0, 1)
    n = x.shape[0]
    buf = np.concatenate([sv, x[:, :, 0]])
    acc = get(inp.taps, buf, n, 2 * m + odd, sym)
    sv[:] = buf[n:]
    return (acc + buf[m:m + n] if odd and sym else acc)[:, :, None]


def restate_hbf(case, inp, x, sv):
    """hbf.rs:163-185 (`HbfDec`: even[m-1] ++ odd[2m-1]) and :207-227 (`HbfInt`: x[2m-1]), stage after stage."""
    kind = case.hbf[0]
    frames, L, r = x.shape
    cur, off = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(frames * r, L), 0
    for taps in inp.taps:
        m = len(taps)
        if kind == "dec":
            n = cur.shape[0] // 2
            even = np.concatenate([sv[off:off + m - 1], cur[0::2]])
            oddb = np.concatenate([sv[off + m - 1:off + 3 * m - 2], cur[1::2]])
            out = get(taps, oddb, n, 2 * m) + even[:n]
            sv[off:off + m - 1], sv[off + m - 1:off + 3 * m - 2] = even[n:], oddb[n:]
            off += 3 * m - 2
        else:
            n = cur.shape[0]
            xb = np.concatenate([sv[off:off + 2 * m - 1], cur])
            out = np.empty((2 * n, L), cur.dtype)
            out[0::2], out[1::2] = get(taps, xb, n, 2 * m), xb[m:m + n]
            sv[off:off + 2 * m - 1] = xb[n:]
            off += 2 * m - 1
        cur = out
    rout = case.rout
    return np.ascontiguousarray(cur.reshape(frames, rout, L).transpose(0, 2, 1))


def restate(case, inp, lanes):
    """[(y, state values)] of the two calls on the chosen lanes."""
    sv = S.state_values(inp.state, case.dtype)[:, lanes].copy()
    out = []
    with np.errstate(all="ignore"):
        for x, lo in zip(inp.x, inp.lo):
            x = x[:, lanes]
            if case.call == "cfg":
                y = restate_hbf(case, inp, x, sv) if getattr(case, "hbf", None) else restate_fir(case, inp, x, sv)
            else:
                y = restate_iir(case, inp, x, None if lo is None else lo[:, lanes], sv, lanes)
            out.append((y, sv.copy()))
    return out


def entries(table):
    ops = []
    for c in S.TABLES[table]():
        key = c.op + ("_bylane" if c.call == "bylane" else "")
        if key not in ops:
            ops.append(key)
    return ops


PARAMS = [(t, op) for t in S.TABLES for op in entries(t)]


def entry_cases(table, entry):
    cases = [c for c in S.TABLES[table]() if c.op + ("_bylane" if c.call == "bylane" else "") == entry]
    assert cases and all(c.kernel for c in cases)  # every case names the kernel family it is there for
    return cases


def check_case(case):
    """One case: the conditions on the oracle, then oracle against restatement on outputs and state of both calls."""
    inp = S.prepare(case)
    res = S.run_oracle(case, inp)
    census = S.check_conditions(case, inp, res)
    lanes = np.arange(min(case.lanes, RESTATE_LANES) if case.lanes > 4096 else case.lanes)
    for rep, ((yo, so), (yr, sr)) in enumerate(zip(res, restate(case, inp, lanes))):
        yo, svo = np.ascontiguousarray(yo[:, lanes]), S.state_values(so, case.dtype)[:, lanes]
        S.assert_same_float(yr, yo, f"{case.id} call {rep}: oracle vs restatement", S.where(case, inp, yo.shape))
        S.assert_same_float(sr, svo, f"{case.id} call {rep}: oracle state vs restatement", S.where(case, inp, svo.shape))
    return census


@pytest.mark.parametrize("table,entry", PARAMS, ids=[p[1] for p in PARAMS])
def test_oracle_meets_restatement_and_conditions(table, entry):
    t0 = time.time()
    union = {"inf": 0, "subnormal": 0, "+0": 0, "-0": 0}
    cases = entry_cases(table, entry)
    failed = []  # every case runs, so that one failing case does not hide the others
    for case in cases:
        try:
            census = check_case(case)
        except AssertionError as e:
            failed.append(str(e)[:400])
            continue
        for k in union:
            union[k] += census[k]
    assert not failed, (len(failed), failed[:10])
    assert all(v > 0 for v in union.values()), (entry, union)
    print(f"{entry}: {len(cases)} cases, {union}, {time.time() - t0:.1f} s")


def test_assert_same_float_rule():
    """+0 / -0 and a one-bit subnormal difference are differences; NaN sign and payload are not; NaN against a number is."""
    for dt, u in ((np.float32, np.uint32), (np.float64, np.uint64)):
        a = np.array([0.0, -0.0, 1.0, np.nan, np.inf], dt)
        S.assert_same_float(a, a.copy(), "same")
        b = a.copy()
        b.view(u)[3] ^= u(1) << u(8 * a.itemsize - 1)  # NaN of the other sign
        b.view(u)[3] |= u(5)                           # ... and another payload
        S.assert_same_float(a, b, "NaN bits")
        for i, v in ((0, -0.0), (1, 0.0), (3, 1.0), (2, np.nan), (4, np.finfo(dt).max)):
            b = a.copy()
            b[i] = v
            with pytest.raises(AssertionError, match="first at flat index %d" % i):
                S.assert_same_float(a, b, "differs")
        s = np.array([1, 2], u).view(dt)  # two neighbouring subnormals
        with pytest.raises(AssertionError):
            S.assert_same_float(s[:1], s[1:], "subnormal")
        assert not (S.bits(S.poison(4, dt)) != S.POISON[dt]).any() and np.isfinite(S.poison(4, dt)).all()
        with pytest.raises(AssertionError):
            S.assert_poison_absent(S.poison(1, dt), "poison")


def test_generator_keeps_one_kind_per_lane():
    rng = np.random.default_rng(1)
    for dt in (np.float32, np.float64):
        x, kind = S.special_chunks(rng, 70, 64, 16, dt)
        assert x.shape == (70, 64, 16) and np.array_equal(kind, np.arange(64) % 8)
        per = [S.classes(x[:, kind == k]) for k in range(8)]
        assert per[0]["normal"] == x[:, kind == 0].size
        assert per[1]["+0"] + per[1]["-0"] == x[:, kind == 1].size and per[1]["+0"] and per[1]["-0"]
        assert per[2]["subnormal"] == x[:, kind == 2].size
        assert per[3]["normal"] == x[:, kind == 3].size and np.abs(x[:, kind == 3]).min() >= 1e30
        assert per[4]["inf"] == 8 and per[5]["nan"] * x[:, kind == 5].size == pytest.approx(8)
        assert per[6]["normal"] + per[6]["subnormal"] == x[:, kind == 6].size and np.abs(x[:, kind == 6]).max() < 1e-36 * (1 if dt == np.float32 else 1e-270)
        assert all(per[7][k] for k in ("+0", "-0", "subnormal", "normal"))
        st = S.special_state(rng, 8, 64, kind, dt)
        assert st.dtype == np.uint32 and st.shape == (8, 64)
        assert np.array_equal(S.state_words(S.state_values(st, dt)), st)


def test_restatement_agrees_with_spec_on_special_values():
    """oracle/spec.py restates the f32 sections on scalars (its clamp is an `if`, so it cannot run elementwise over lanes,
    which is why the table above uses the restatement of this file): the two agree lane by lane on special data."""
    from oracle import spec

    rng = np.random.default_rng(7)
    x, kind = S.special_x(rng, 40, 16, np.float32)
    ba = [np.float32(v) for v in rng.uniform(-0.5, 0.5, 5)]
    for cl in (None, (-0.0, -np.inf, np.inf), (0.01, -0.0, 0.0), (0.05, -0.7, 0.9)):
        clf = None if cl is None else [np.float32(v) for v in cl]
        with np.errstate(all="ignore"):
            y1 = df1_section(ba, clf, [np.zeros(16, np.float32) for _ in range(4)], x)
            y2 = df2t_section(ba, clf, [np.zeros(16, np.float32) for _ in range(2)], x)
            for lane in range(16):
                st, s2 = spec.DirectForm1(np.float32(0)), [np.float32(0), np.float32(0)]
                if cl is None:
                    w1 = [spec.biquad_f32_df1(ba, st, v) for v in x[:, lane]]
                    w2 = [spec.biquad_f32_df2t(ba, s2, v) for v in x[:, lane]]
                else:
                    w1 = [spec.biquad_f32_df1_clamp(ba, *cl, st, v) for v in x[:, lane]]
                    w2 = [spec.biquad_f32_df2t_clamp(ba, *cl, s2, v) for v in x[:, lane]]
                S.assert_same_float(np.array(w1, np.float32), y1[:, lane], f"df1 {cl} lane {lane} kind {kind[lane]}")
                S.assert_same_float(np.array(w2, np.float32), y2[:, lane], f"df2t {cl} lane {lane} kind {kind[lane]}")
