"""CPU checks of the exact-data sweep over the Winograd F(4x4) kernels (tests/wino4_exact_cases.py): the conditions that make
bit equality with float64 a theorem (every sum and result below 2^24 granules, recomputed here from first principles), that make
each case a test (coverage conditions, non-zero outputs, distinct channels) and that ONE thing done wrong in the reference
changes the expected output. Run with -s for the ledger of every case."""
import dataclasses
from fractions import Fraction

import numpy as np
import pytest

import wino4_exact_cases as C

_ID = lambda c: c.id
SMALL = [c for c in C.ALL_CASES if c.b * c.h * c.w * c.cout <= 2 * 20 * 28 * 128]


def test_the_restated_matrices_are_the_algorithm():
    """B^T and A^T as restated from the kernel's comments, with G from the interpolation points, compute a 3x3 convolution
    (exact rational arithmetic): the second statement is one of F(4x4, 3x3), and its denominators are the issue's."""
    assert C.BT_DEN.tolist() == [64, 16, 16, 32, 32, 64]
    rng = np.random.default_rng(7)
    fr = np.vectorize(lambda v: Fraction(float(v)), otypes=[object])
    g, d = fr(rng.integers(-3, 4, (3, 3))), fr(rng.integers(-4, 5, (6, 6)))
    gm, bt, at = np.array(C.g_matrix(), dtype=object), fr(C.BT), fr(C.AT)
    y = at.dot((gm.dot(g).dot(gm.T)) * (bt.dot(d).dot(bt.T))).dot(at.T)
    want = [[sum(d[i + ky, j + kx] * g[ky, kx] for ky in range(3) for kx in range(3)) for j in range(4)] for i in range(4)]
    assert y.tolist() == want
    # G . 243 is integer: the denominators of G g G^T divide 3^10
    assert all((v * 243).denominator == 1 for row in C.g_matrix() for v in row)


# the issue's table: the largest K = sum_c |U_c| under 2^24 granules at the worst pixel, |d| <= 1
K_TABLE = {("E", "E"): 158, ("3/4", "E"): 21, ("3/2", "E"): 15, ("3/4", "3/4"): 2, ("3/2", "3/4"): 2, ("3/2", "3/2"): 1}


def test_the_budget_table_from_first_principles():
    """A patch of ones through |B^T| . |B| and |A^T| . |A| with a one-hot U, by brute force over all 36 components and 16
    pixels, in granules of 1 / (den B^T[xi] den B^T[nu] den A^T[i][xi] den A^T[j][nu])."""
    vabs = np.abs(C.BT) @ np.ones((6, 6)) @ np.abs(C.BT).T
    seen = {}
    for xi in range(6):
        for nu in range(6):
            m = np.zeros((6, 6))
            m[xi, nu] = vabs[xi, nu]
            y = np.abs(C.AT) @ m @ np.abs(C.AT).T
            worst = 0.0
            for i in range(4):
                for j in range(4):
                    if y[i, j]:
                        den = Fraction(float(C.BT_DEN[xi] * C.BT_DEN[nu])) * Fraction(float(C.AT[i, xi])).denominator * \
                            Fraction(float(C.AT[j, nu])).denominator
                        worst = max(worst, float(Fraction(float(y[i, j])) * den))
            k = int((2 ** 24 - 1) // worst)
            assert k == C.k_table(xi, nu), (xi, nu)
            key = tuple(sorted((C.point_class(xi), C.point_class(nu))))
            assert seen.setdefault(key, k) == k
            assert C.fits(xi, nu, k) and not C.fits(xi, nu, k + 1)
    assert seen == K_TABLE, seen


@pytest.mark.parametrize("case", C.ALL_CASES, ids=_ID)
def test_case_is_exact_and_discriminating(case):
    d = C.build(case)
    bits = d.budget.bits()
    print(f"\n{case.id}: K {int(d.k.min())}..{int(d.k.max())}; bits " + ", ".join(f"{k} {v:.2f}" for k, v in bits.items()))
    for name, v in bits.items():
        assert v < 24.0, (case.id, name, f"{v:.2f} bits: may not be exact in fp32")
    # the data rule: |x| <= 1, integer U with one component per channel, K within the table, power-of-two scales, shifts that
    # are multiples of the channel's finest granule
    assert set(np.unique(d.x)) <= {-1.0, 0.0, 1.0}
    assert np.array_equal(d.u, np.round(d.u)) and np.array_equal(np.abs(d.u).sum((1, 2, 3)), d.k)
    for o in range(case.cout):
        xi, nu = d.comp[o]
        assert 1 <= d.k[o] <= C.k_table(xi, nu), (case.id, o)
        fine = C.G_OUT[xi, nu][C.LIVE[xi, nu]].min() * d.scale[o]
        assert (d.shift[o] / fine) == round(d.shift[o] / fine) and np.log2(d.scale[o]) == round(np.log2(d.scale[o]))
    # every reference value is an integer number of its granule
    b, gh, gw, n = d.acc.shape
    tiles = d.acc.reshape(b, gh // 4, 4, gw // 4, 4, n).transpose(0, 1, 3, 2, 4, 5)
    g_out = C.G_OUT[d.comp[:, 0], d.comp[:, 1]].transpose(1, 2, 0)
    q = tiles / g_out
    assert np.array_equal(q, np.round(q)) and float(np.abs(q).max()) < 2 ** 24
    for key, w64 in d.want64.items():
        for t64, t32 in zip(*[v if isinstance(v, tuple) else (v,) for v in (w64, d.want[key])]):
            assert t32.dtype == np.float32 and np.array_equal(t32.astype(np.float64), t64), (case.id, key, "not an fp32 value")
            assert np.isfinite(t64).all() and not np.signbit(t64[t64 == 0]).any(), (case.id, key, "inf or -0 in the reference")
    assert C.data_problems(case, d) == []
    if case.form == "heads":
        raw, nhwc = d.want64[(True, True)]
        assert raw.shape == (case.b * np.prod(C.grid(case.h, case.w)) * 512, 32) and not raw[:, 18:].any()
        assert nhwc.shape == (case.b, case.h, case.w, 18)
    cut = float((d.pre <= 0).mean())
    print(f"    {cut:.2f} <= 0 before the ReLU")
    assert 0.2 <= cut <= 0.8, (case.id, cut)


@pytest.mark.parametrize("case", SMALL, ids=_ID)
def test_fp32_in_two_summation_orders_equals_float64(case):
    o = C.operands(case)
    want = C.bilinear(o["x"], o["u"])
    for reverse in (False, True):
        got = C.bilinear32(o["x"], o["u"], reverse)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), (case.id, reverse)


def test_case_table_covers_what_it_promises():
    assert C.coverage_problems() == []
    ids = [c.id for c in C.ALL_CASES]
    assert len(set(ids)) == len(ids)
    for gone in ("w4-plain-1x4x4x8x64", "w4-plain-2x20x28x24x128", "w4-heads-2x36x40x16x256", "w4-heads-1x96x96x8x128",
                 "w4-conv3-1x20x44x16x64-c3_96", "w4-conv3-2x4x4x8x64-c3_256"):
        assert gone in ids
        assert C.coverage_problems([c for c in C.ALL_CASES if c.id != gone]), gone
    assert C.coverage_problems([c for c in C.ALL_CASES if c.tag != "clamp"])


@pytest.mark.parametrize("form", ["plain", "heads", "conv3"])
def test_mutants_of_the_reference_change_the_expected_output(form):
    """Each mutant, in EVERY case of the form it applies to (last_image: more than one image), changes at least one element."""
    seen = {}
    for case in [c for c in C.ALL_CASES if c.form == form]:
        o = C.operands(case)
        nhwc = lambda want: want[1] if isinstance(want, tuple) else want
        if case.tag == "clamp":
            # 261 M tiles of i.i.d. data: the mutants run on the first two M tiles, compared on the 56 columns whose patches
            # end inside them — there the narrow form IS the wide one (asserted), so what changes it changes the wide case
            wide = nhwc(C.build(case).want64[(True, True)])
            case, o = dataclasses.replace(case, w=64, tag=""), dict(o, x=np.ascontiguousarray(o["x"][:, :, :64]))
            ref = nhwc(C.evaluate(case, o)["want"])[:, :, :56].ravel()
            assert np.array_equal(ref, wide[:, :, :56].ravel())
            flat = lambda want: nhwc(want)[:, :, :56].ravel()
        else:
            flat = C.flat
            ref = flat(C.evaluate(case, o)["want"])
            assert np.array_equal(ref, flat(C.build(case).want64[(True, True)]))
        for mut in C.mutants_of(case):
            n = int((flat(C.mutant_want(case, o, mut)) != ref).sum())
            assert n > 0, f"{case.id}: the data do not notice the mutant {mut}"
            seen[mut] = seen.get(mut, 0) + 1
    assert set(seen) == set(C.MUTANTS) | set(C.FORM_MUTANTS[form])
    print(f"\n{form}: " + ", ".join(f"{m} x{n}" for m, n in sorted(seen.items())))


@pytest.mark.parametrize("cout,cin", C.WEIGHT_SHAPES)
def test_filter_data_are_exact_in_fp32(cout, cin):
    """g = 3^10 * {-2..2} * 2^k: G g G^T in rational arithmetic is a short dyadic number — an fp32 value, and so is every
    intermediate of the kernel's double evaluation (integers below 2^53)."""
    g, u = C.weights_int(cout, cin)
    assert np.array_equal(g.astype(np.float32).astype(np.float64), g)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert np.count_nonzero(u) >= 0.5 * u.size and float(np.abs(u).max()) < 2 ** 24 * 4
    assert C.u_layout(u).shape == (cin // 4, 36, 2, cout, 2)
    # the layout: channel c of output n, component k sits at [c / 4][k][(c / 2) % 2][n][c % 2]
    lay = C.u_layout(u)
    for n, k, c in ((0, 0, 0), (cout - 1, 35, cin - 1), (cout // 2, 17, 2), (0, 7, 1)):
        assert lay[c // 4, k, (c // 2) % 2, n, c % 2] == u[n, k // 6, k % 6, c]


def test_round_f32_rounds_once():
    fr = Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)       # through float64: a tie, to even, 1.0; once: the upper value
    assert C.round_f32(fr) == np.nextafter(np.float32(1), np.float32(2))
    assert np.float32(float(fr)) == np.float32(1)
