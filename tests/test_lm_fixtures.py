"""Host checks of tests/lm_fixtures.py, the reference of test_gpu_lm_linear.py: the bounds hold with margin for LAPACK's
own factor and solutions on every fixture (they are not too tight), every fixture's exact factor stays inside its
envelope, the restated plan agrees with what the fixtures claim to exercise, and a slightly wrong factor breaks the
bounds (they are not too loose)."""
import numpy as np
import pytest

import lm_fixtures as F

MARGIN = 0.5  # LAPACK must use at most half of every bound

CASES = F.all_cases() + [F.column_order_case(512)]


def _pd(c):
    return c.ref["L"] is not None


@pytest.mark.parametrize("case", CASES, ids=str)
def test_lapack_meets_the_bounds_with_margin(case):
    c = case
    if c.expect in ("fail", "nan_g"):
        assert not _pd(c)
        return
    assert _pd(c), c.name
    r, n = c.ref, c.n
    Wa = r["W"]
    assert F.factor_ratio(Wa, r["L"], c.plan["stored"]) <= MARGIN
    assert F.forward_ratio(r["L"], r["y"], Wa[n]) <= MARGIN
    assert F.backward_ratio(Wa, r["x"]) <= MARGIN
    s1 = 0.5 * float(np.sum(r["x"] * Wa[n] + F.lm_diag(c) * r["x"] ** 2))
    assert F.model_ratio(c, r["x"], s1) <= MARGIN
    if c.well:
        assert F.kappa(Wa) < 1e4, c.name
        assert F.forward_error_ratio(Wa, r["x"], r["x"] * (1 + F.U)) <= MARGIN


def test_big_case_meets_the_bounds():
    c = F.big_case()
    r = c.ref
    assert F.factor_ratio(r["W"], r["L"], c.plan["stored"]) <= MARGIN
    assert F.backward_ratio(r["W"], r["x"]) <= MARGIN


@pytest.mark.parametrize("case", CASES + [F.big_case()], ids=str)
def test_exact_factor_inside_the_envelope(case):
    c = case
    low = np.tril(c.A) != 0
    assert not (low & ~c.mask).any()
    if _pd(c):
        assert not ((c.ref["L"] != 0) & ~c.mask).any()


def test_conditioning_cases():
    by = {c.name: c for c in F.all_cases()}
    assert 3e7 < F.kappa(by["kappa8_n193"].ref["W"]) < 3e9
    assert 3e11 < F.kappa(by["kappa12_n193"].ref["W"]) < 3e13
    assert F.kappa(by["near_singular_point_n12"].ref["W"]) > 1e11
    g = by["graded_n193"]
    assert g.diagonal.min() <= 1e-6 * 1.01 and g.diagonal.max() >= 1e31
    # the damped singular case: A itself is singular, W is not
    s = by["singular_psd_damped_n129"]
    assert np.linalg.matrix_rank(s.A) < s.n and _pd(s)


def test_plan_reaches_every_claim_order_and_edge():
    """the fixtures cover: n % 64 in {0, 1, 15, 16, 17, 63}; the augmented row inside and beyond the last diagonal tile; a
    tail that starts mid-block; tail_begin == n; a non-monotone env_end; 2 and 3 regions with a folded last region; and
    each claim order on a device with 512 or 1024 slots"""
    cases = F.all_cases()
    assert {c.n % 64 for c in cases} >= {0, 1, 15, 16, 17, 63}
    assert any(c.n % 64 == 0 for c in cases) and any(c.n % 64 != 0 for c in cases)  # row n: own block / last tile
    assert any(c.tail_begin % 64 == 17 for c in cases)
    assert any(c.tail_begin == c.n and c.n % 64 for c in cases)
    assert any(any(b < a for a, b in zip(c.env_end, c.env_end[1:])) for c in cases)
    regions = {c.name: c.plan for c in cases if c.region_begin}
    assert sorted(p["regions"] for p in regions.values()) == [2, 3]
    folded = regions["regions3_folded_n468"]
    assert folded["region_bounds"] == [0, 2, 3, 6] and 1 in np.diff(folded["region_bounds"])
    for slots in (512, 1024):
        orders = {F.plan(c.n, c.env_end, c.tail_begin, c.region_begin, slots)["order"]
                  for c in cases + [F.big_case(), F.column_order_case(slots)]}
        assert orders == {0, 1, 2}
    # the non-monotone envelope: the plan stores the fill the input envelope leaves out
    c = {c.name: c for c in cases}["nonmonotone_n193"]
    assert c.plan["bend"] == [3, 3, 3, 4] and (c.ref["L"][128:192, 64:128] != 0).any()


def _perturbed_ratios(c):
    r = c.ref
    Wa, L, stored = r["W"], r["L"].copy(), c.plan["stored"]
    # one off-diagonal tile 1e-10 relative off
    I, J = next((I, J) for J in range(stored.shape[1]) for I in range(J + 1, stored.shape[1]) if stored[I, J])
    L1 = L.copy()
    L1[I * 64:(I + 1) * 64, J * 64:(J + 1) * 64] *= 1 + 1e-10
    # one term of one trailing update dropped: L_ij computed without its largest term L_ik L_jk
    rows, cols = slice(I * 64, min((I + 1) * 64, c.n)), slice(J * 64, (J + 1) * 64)
    prod = np.abs(L[rows, None, :] * L[None, cols, :])  # [i, j, k]
    j_of = np.arange(J * 64, J * 64 + prod.shape[1])
    prod *= np.arange(prod.shape[2])[None, None, :] < j_of[None, :, None]  # k < j: a term of the update of L_ij
    a, b, k = np.unravel_index(np.argmax(prod), prod.shape)
    i, j = I * 64 + a, J * 64 + b
    L2 = L.copy()
    L2[i, j] += L[i, k] * L[j, k] / L[j, j]
    return F.factor_ratio(Wa, L1, stored), F.factor_ratio(Wa, L2, stored)


@pytest.mark.parametrize("name", ["dense_tail_n193", "band_tail65_n193", "regions2_n330", "kappa12_n193", "graded_n193"])
def test_a_slightly_wrong_factor_breaks_the_bound(name):
    c = {c.name: c for c in F.all_cases()}[name]
    tile, term = _perturbed_ratios(c)
    assert tile > 1.0 and term > 1.0, (tile, term)
