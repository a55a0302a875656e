"""CPU: the restatement of TV-L1 optical flow (tests/tvl1_ref.py) against itself and on real data -- its two statements of the iteration
and of the rc stage, the properties the kernels stand on (zero duals on the last row and column, a dependency radius of one pixel per
iteration), the degenerate inputs, and the Yosemite pair with the driver's defaults.

Recorded (this file, the defaults, 11 scales): Yosemite AEE 0.332 px over all pixels and 0.107 px below the cloud band, correlations 0.964
(U) and 0.928 (V); with 5 % of frame 1 replaced by uniform noise and lambda = 10: 0.377 / 0.219."""
import numpy as np

import problems as pb
import tvl1_cases as tc
import tvl1_ref as ref

F32 = np.float32


def same(got, want, what):
    assert pb.bit_equal(np.asfortranarray(got), np.asfortranarray(want)), "%s: %s" % (what, pb.describe_mismatch(np.asfortranarray(got), np.asfortranarray(want)))


def test_the_two_statements_agree():
    for shape in ((1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (13, 11)):
        for lam, huber, it, holes, inf, with_P in ((15.0, 0.0, 3, "none", False, False), (40.0, 0.05, 4, "scattered", False, True),
                                                   (0.0, 0.0, 2, "corner", True, True), (1.0e4, 0.05, 3, "all", False, False)):
            rc, gx, gy, U, V, P = tc.planes(shape, 5, holes, inf)
            c = ref.Consts(lam, huber)
            a = ref.iterate(rc, gx, gy, U, V, c, it, P if with_P else None)
            b = ref.iterate(rc, gx, gy, U, V, c, it, P if with_P else None, stepper=ref.step_loops)
            for k, (x, y) in enumerate(zip(a, b)):
                same(x, y, "%s %s plane %d" % (shape, (lam, huber, it, holes, inf, with_P), k))
        I0, W, gx, gy, U0, V0, rc = tc.rc_case(shape)
        same(ref.rc_stage_loops(I0, W, gx, gy, U0, V0), rc, "rc %s" % (shape,))
        assert np.isnan(rc).any() or shape == (1, 1)


def test_duals_are_zero_on_the_last_row_and_column():
    for shape in ((1, 1), (1, 9), (9, 1), (13, 11)):
        rc, gx, gy, U, V, P = tc.planes(shape, 5, "scattered")
        for with_P in (False, True):
            for huber in (0.0, 0.05):
                s = ref.iterate(rc, gx, gy, U, V, ref.Consts(15.0, huber), 5, P if with_P else None)
                for px, py in ((s[4], s[5]), (s[6], s[7])):
                    assert (px[-1, :] == 0).all() and (py[:, -1] == 0).all() and not np.signbit(px[-1, :]).any() and not np.signbit(py[:, -1]).any()


def test_a_pixel_depends_on_nothing_farther_than_one_pixel_per_iteration():
    """Change every input farther than T pixels (Chebyshev) from a probe: all eight state planes keep their bits at the probe after T
    iterations.  A blocked kernel with a halo of T stands on this; so does the single step's recomputation of its neighbours."""
    shape = (23, 21)
    rc, gx, gy, U, V, P = tc.planes(shape, 5, "scattered")
    rng = np.random.default_rng(3)
    i, j = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    for probe in ((11, 10), (0, 0), (22, 20), (5, 20)):
        for T in (1, 2, 3, 4):
            far = np.maximum(np.abs(i - probe[0]), np.abs(j - probe[1])) > T
            other = [np.where(far, rng.uniform(-3.0, 3.0, shape).astype(F32), a) for a in (rc, gx, gy, U, V)]
            other[0][far & (rng.random(shape) < 0.2)] = np.nan
            Pother = [np.where(far, rng.uniform(-0.4, 0.4, shape).astype(F32), a) for a in P]
            for huber in (0.0, 0.05):
                c = ref.Consts(15.0, huber)
                a = ref.iterate(rc, gx, gy, U, V, c, T, P)
                b = ref.iterate(*other, c, T, Pother)
                for k in range(8):
                    assert a[k][probe].tobytes() == b[k][probe].tobytes(), (probe, T, huber, k)
            # and the radius is tight: a change T pixels away is felt
        near = (np.abs(i - 11) == 4) & (np.abs(j - 10) <= 4)
        moved = np.where(near, U + F32(1.0), U)
        assert ref.iterate(rc, gx, gy, moved, V, ref.Consts(15.0), 4, P)[0][11, 10] != ref.iterate(rc, gx, gy, U, V, ref.Consts(15.0), 4, P)[0][11, 10]


def test_a_constant_pair_gives_exactly_zero_flow(oracle):
    I = np.full((40, 52, 2), 93.0, F32)
    U, V = ref.flow_tvl1(oracle, I)
    assert U.shape == (40, 52) and (U == 0).all() and (V == 0).all()
    z = np.zeros((9, 7), F32)
    s = ref.iterate(z, z, z, z, z, ref.Consts(15.0), 6)
    assert all((x == 0).all() and not np.signbit(x).any() for x in s)


def test_pixels_without_data_take_the_pure_tv_step():
    shape = (13, 11)
    rc, gx, gy, U, V, P = tc.planes(shape, 5, "all")
    for huber in (0.0, 0.05):
        got = ref.iterate(rc, gx, gy, U, V, ref.Consts(15.0, huber), 4, P)
        # lambda = 0 on data that could pull: the thresholding step vanishes and leaves a + (+-0) * g
        rc0 = tc.planes(shape, 5, "none")[0]
        want = ref.iterate(rc0, gx, gy, U, V, ref.Consts(0.0, huber), 4, P)
        for k in range(8):
            same(got[k], want[k], "plane %d" % k)
    # a mixed plane: the NaN pixels' update is a = u + tau div p' exactly
    rc, gx, gy, U, V, P = tc.planes(shape, 5, "scattered")
    c = ref.Consts(15.0)
    one = ref.iterate(rc, gx, gy, U, V, c, 1, P)
    pure = ref.iterate(np.full(shape, np.nan, F32), gx, gy, U, V, c, 1, P)
    hole = np.isnan(rc)
    assert hole.any() and (one[0][hole] == pure[0][hole]).all() and (one[1][hole] == pure[1][hole]).all()
    assert (one[0][~hole] != pure[0][~hole]).any()
    for k in range(4, 8):
        same(one[k], pure[k], "the duals do not see rc")


def test_yosemite_with_the_defaults(oracle):
    _, Ut, Vt = tc.yosemite()
    U, V = tc.yosemite_flow(oracle)
    e = tc.errors(U, V, Ut, Vt)
    print("Yosemite, defaults: AEE %.3f, below the cloud band %.3f, corr U %.3f, corr V %.3f" % e)
    assert e[0] < 0.5 and e[1] < 0.2, e
    assert e[2] > 0.9 and e[3] > 0.85, e


def test_yosemite_with_outliers_stays_finite(oracle):
    _, Ut, Vt = tc.yosemite()
    U, V = tc.yosemite_flow(oracle, outliers=True)
    assert np.isfinite(U).all() and np.isfinite(V).all()
    e = tc.errors(U, V, Ut, Vt)
    print("Yosemite, 5 %% outliers, lambda 10: AEE %.3f, below the cloud band %.3f" % e[:2])
    assert e[0] < 0.5, e


def test_random_pairs_stay_finite(oracle):
    rng = np.random.default_rng(2)
    for shape in ((24, 31), (21, 40)):
        U, V = ref.flow_tvl1(oracle, rng.uniform(0.0, 255.0, shape + (2,)).astype(F32))
        assert np.isfinite(U).all() and np.isfinite(V).all()
