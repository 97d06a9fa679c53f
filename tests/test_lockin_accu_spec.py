"""The specification of idsp_lockin_i32_accu_process, held to a second restatement (no GPU): `accu_lo_np` fed to the checker
library's lockin_i32_lo_process (tests/_lockin_accu_cases.py, spec) against a per-sample walk in Python integers on
oracle/spec.py (per_sample_int) — every output word and every state word, for every (order, cascade) and k in {0, 1, 3}, on
adversarial `Accu` rows (full-range states, steps with the top bit set) and samples that include i32::MIN, i32::MAX and 0."""
import numpy as np
import pytest

from tests import _lockin_accu_cases as LA
from tests import _rpll_spec as S


@pytest.mark.parametrize("order,cascade", LA.SHAPES)
@pytest.mark.parametrize("k", [0, 1, 3])
def test_composition_equals_the_per_sample_walk(order, cascade, k):
    rng = np.random.default_rng(100 * k + 10 * order + cascade)
    lanes, updates = 5, 4
    ks = LA.lowpass_ks(rng, order, cascade)
    h = S.LO_HARMONICS[(k + order + cascade) % len(S.LO_HARMONICS)]
    lo_cfg = (k, h, int(rng.integers(-(1 << 31), 1 << 31)))
    accu = S.adversarial_accu(rng, updates, lanes)
    x = LA.adversarial_x(rng, updates << k, lanes)
    assert {LA.I32_MIN, LA.I32_MAX, 0} <= set(x.reshape(-1).tolist())
    st0 = LA.random_state(rng, order, cascade, lanes)
    sa, sb = st0.copy(), st0.copy()
    ya = LA.spec(ks, lo_cfg, sa, x, accu)
    yb = LA.per_sample_int(ks, lo_cfg, sb, x, accu)
    assert np.array_equal(ya, yb), (order, cascade, lo_cfg)
    assert np.array_equal(sa, sb) and not np.array_equal(sa, st0), (order, cascade, lo_cfg)


def test_every_harmonic_and_chunked_state():
    """every harmonic of the list on one shape; two calls on update ranges carry the state like one"""
    rng = np.random.default_rng(7)
    lanes, updates, k, ks = 4, 6, 1, LA.lowpass_ks(rng, 2, 2)
    accu = S.adversarial_accu(rng, updates, lanes)
    x = LA.adversarial_x(rng, updates << k, lanes)
    for h in S.LO_HARMONICS:
        lo_cfg = (k, h, -12345)
        st0 = LA.random_state(rng, 2, 2, lanes)
        sa, sb, sc = st0.copy(), st0.copy(), st0.copy()
        ya = LA.spec(ks, lo_cfg, sa, x, accu)
        yb = LA.per_sample_int(ks, lo_cfg, sb, x, accu)
        yc = np.concatenate([LA.spec(ks, lo_cfg, sc, x[u0 << k:u1 << k], accu[u0:u1]) for u0, u1 in ((0, 1), (1, 6))])
        assert np.array_equal(ya, yb) and np.array_equal(sa, sb), h
        assert np.array_equal(ya, yc) and np.array_equal(sa, sc), h
