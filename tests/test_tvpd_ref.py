"""CPU: the NumPy restatement of primal-dual total variation (tests/tvpd_ref.py) against itself and against what the issue promises.

  the whole-array statement equals the per-pixel loop bit for bit on the small shapes
  px on the last row and py on the last column stay exactly 0
  TV-L1 returns a constant plane with its own bits; ROF on a 1 x 1 plane does not (the division rounds), pinned as it is
  a change of one pixel of f changes no state farther than T pixels away after T iterations (what k_tvpd_block rests on)
  on the outlier scene TV-L1 is better than a third of the best ROF, with and without a hole"""
import numpy as np
import pytest

import problems as pb
import tvpd_cases as tc
import tvpd_ref

F32 = np.float32
SMALL = [s for s in tc.SHAPES if s[0] * s[1] <= 70]


def same(got, want, what):
    assert pb.bit_equal(got, want), "%s: %s" % (what, pb.describe_mismatch(got, want))


@pytest.mark.parametrize("shape", SMALL, ids=tc.shape_id)
def test_whole_array_equals_the_pixel_loop(shape):
    for model in ("l1", "l2"):
        for huber in (0.0, 0.05):
            for holes in ("none", "scattered"):
                f = tc.plane(shape, 11, holes)
                c = tvpd_ref.Consts(model, 0.8, huber)
                u0 = tvpd_ref.start(f)
                a = tvpd_ref.iterate(f, u0, c, 5)
                b = tvpd_ref.iterate(f, u0, c, 5, tvpd_ref.step_loops)
                for x, y, name in zip(a, b, ("u", "u_prev", "px", "py")):
                    same(x, y, "%s %s huber %g holes %s: %s" % (tc.shape_id(shape), model, huber, holes, name))


def test_the_far_border_of_the_dual_stays_zero():
    for shape in ((1, 1), (1, 70), (70, 1), (3, 5), (37, 21)):
        for model, huber in (("l1", 0.0), ("l2", 0.05)):
            f = tc.plane(shape, 5, "corner" if shape[0] > 1 and shape[1] > 1 else "none")
            c = tvpd_ref.Consts(model, 0.8, huber)
            for iters in (1, 2, 7):
                _, _, px, py = tvpd_ref.iterate(f, tvpd_ref.start(f), c, iters)
                assert (px[-1, :].view(np.uint32) == 0).all() and (py[:, -1].view(np.uint32) == 0).all(), (shape, model, iters)
                if shape[0] > 1 and shape[1] > 1:
                    assert px[:-1, :].any() and py[:, :-1].any()


def test_l1_keeps_a_constant_plane_and_l2_rounds_on_a_single_pixel():
    for value in (0.1, -3.7, 1.0e-30, 12345.678):
        f = np.full((9, 7), value, F32)
        for huber in (0.0, 0.05):
            same(tvpd_ref.tv_pd(f, "l1", 0.8, 10, huber=huber), f, "l1 of the constant %g" % value)
    # (f + tl f) / (1 + tl) with tl = 0.25 * 0.8 in float32: the product and the sum round, and the quotient is one ulp below f
    f = np.full((1, 1), 0.7, F32)
    got = tvpd_ref.tv_pd(f, "l2", 0.8, 1)
    tl = F32(F32(0.25) * F32(0.8))
    assert got[0, 0] == F32(F32(f[0, 0] + F32(tl * f[0, 0])) / F32(F32(1.0) + tl))
    assert got.view(np.uint32)[0, 0] == f.view(np.uint32)[0, 0] - 1 == 0x3F333332, hex(int(got.view(np.uint32)[0, 0]))
    same(tvpd_ref.tv_pd(np.full((1, 1), 0.1, F32), "l2", 0.8, 1), np.full((1, 1), 0.1, F32), "a value the step happens to keep")


@pytest.mark.parametrize("T", (1, 2, 3, 4))
def test_t_iterations_reach_t_pixels(T):
    """One pixel of f changed: after T iterations u, u_prev, px and py are bit-identical farther than T pixels from it (the largest of
    the row and the column distance).  Within T they do differ -- the bound is reached."""
    shape, at = (23, 19), (11, 9)
    i, j = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    far = np.maximum(np.abs(i - at[0]), np.abs(j - at[1])) > T
    for model, huber in (("l1", 0.0), ("l2", 0.0), ("l1", 0.05), ("l2", 0.05)):
        f = np.array(tc.plane(shape, 21))
        g = f.copy()
        g[at] += F32(25.0)
        c = tvpd_ref.Consts(model, 0.8, huber)
        u0 = tvpd_ref.start(f)         # the same start for both: the start is not part of the iteration
        a, b = tvpd_ref.iterate(f, u0, c, T), tvpd_ref.iterate(g, u0, c, T)
        for x, y, name in zip(a, b, ("u", "u_prev", "px", "py")):
            assert np.array_equal(x.view(np.uint32)[far], y.view(np.uint32)[far]), "%s %s T %d: a change beyond T pixels" % (model, name, T)
        assert not np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    reach = np.maximum(np.abs(i - at[0]), np.abs(j - at[1]))[a[0].view(np.uint32) != b[0].view(np.uint32)].max()
    assert reach <= T


def test_quality_on_the_outlier_scene():
    """TV-L1 at lambda 0.8 against the best ROF over the issue's lambdas, 300 iterations each: below one third, with and without the
    hole, and finite everywhere."""
    clean, noisy = tc.scene()
    rof = {lam: tc.rms(tvpd_ref.tv_pd(noisy, "l2", lam, tc.QUALITY_ITER), clean) for lam in tc.ROF_LAMBDAS}
    best = min(rof.values())
    l1 = tc.rms(tc.scene_l1(), clean)
    print("noisy %.3f; ROF %s; TV-L1 %.3f; ratio %.3f" % (tc.rms(noisy, clean), " ".join("%g: %.3f" % kv for kv in rof.items()), l1, l1 / best))
    assert l1 < best / 3.0
    holed = tc.scene_l1(hole=True)
    assert np.isnan(tc.scene(hole=True)[1]).sum() == 400 and np.isfinite(holed).all()
    l1h = tc.rms(holed, clean)
    print("TV-L1 with the hole %.3f; ratio %.3f" % (l1h, l1h / best))
    assert l1h < best / 3.0
