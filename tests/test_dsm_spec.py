"""The two restatements of `Dsm<K>` in tests/_dsm_spec.py against each other and against what the reference documents: its doctest
(src/dsm.rs:11-20), the output range of the doc comment, an exact sum invariant, the untouched `c[K-1]`.  No GPU, no library."""
import numpy as np
import pytest

from tests import _dsm_spec as S

ORDERS = list(range(S.MAX_ORDER + 1))
FRAMES, LANES = 500, 50


def _scalar_run(order, st, x):
    """the scalar class over [frames, lanes]: outputs, final state words (as dsm_np leaves them), i8 wraps"""
    frames, lanes = x.shape
    y = np.zeros((frames, lanes), np.int8)
    out = st.copy()
    wraps = 0
    for lane in range(lanes):
        d = S.Dsm(order, a=st[:order, lane], c=[int(w) & 0xFF for w in st[order:, lane]])
        for f in range(frames):
            y[f, lane] = d.process(int(x[f, lane]))
        wraps += d.wraps
        out[:order, lane] = d.a
        for j in range(order - 1):
            out[order + j, lane] = d.c[j] & 0xFFFFFFFF
        if order:
            assert d.c[order - 1] == S._i8(int(st[2 * order - 1, lane]))  # `take(K - 1)`: never read or written
    return y, out, wraps


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("start", ["zero", "random"])
def test_restatements_agree(order, start):
    rng = np.random.default_rng(100 + order)
    x = S.inputs(rng, FRAMES, LANES)
    st = np.zeros((2 * order, LANES), np.uint32) if start == "zero" else S.random_state(rng, order, LANES)
    y_s, st_s, wraps = _scalar_run(order, st, x)
    st_v = st.copy()
    y_v = S.dsm_np(order, st_v, x)
    assert np.array_equal(y_s, y_v) and np.array_equal(st_s, st_v)
    if order:
        assert np.array_equal(st_v[2 * order - 1], st[2 * order - 1])  # c[K-1] comes back untouched, upper bytes included
    if order == 0:
        assert not y_v.any()
    if start == "zero":
        # the documented range, and nothing a debug build would panic on
        assert wraps == 0
        if order:
            assert y_v.min() >= 1 - (1 << (order - 1)) and y_v.max() <= 1 << (order - 1)
    elif order >= 3:
        assert wraps >= 1, "the random-state case must exercise the i8 wrap of the second fold"


def test_reference_doctest():
    """`Dsm::<3>::default()`, x = 0x87654321, n = 2^20: |mean(y) / (x / 2^32) - 1| < n^-1/2 (:11-20)"""
    d = S.Dsm(3)
    x, n = 0x87654321, 1 << 20
    total = 0
    for _ in range(n):
        total += d.process(x)
    assert d.wraps == 0
    assert abs((total / n) / (x / 2.0 ** 32) - 1.0) < n ** -0.5


@pytest.mark.parametrize("order", ORDERS[1:])
def test_sum_invariant(order):
    """from `Dsm::default()` with constant x: sum(y[0..n)) == ((n * x) >> 32) + c[K-2] (the tail term is 0 for K = 1)"""
    xs = [0x87654321, 0, 1, 0xFFFFFFFF, 0x80000000, 0x12345678, 0xDEADBEEF]
    for n in (1, 2, 3, 7, 64, 1000):
        st = np.zeros((2 * order, len(xs)), np.uint32)
        y = S.dsm_np(order, st, np.tile(np.array(xs, np.uint32), (n, 1)))
        tail = st[2 * order - 2].view(np.int32).astype(np.int64) if order >= 2 else 0
        assert np.array_equal(y.astype(np.int64).sum(0), ((n * np.array(xs, np.uint64)) >> np.uint64(32)).astype(np.int64) + tail), (order, n)
