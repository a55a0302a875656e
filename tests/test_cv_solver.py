"""CPU: the Chan-Vese AOS step (CV_solver_2d) at the boundary, and its numpy restatement (cv_ref.py) on its own.

The restatement is what tests/test_gpu_cv.py compares the GPU with bit for bit.  Here it is pinned to the reference's own C
through tests/golden/levelset/cv_solver.npz (inputs and the outputs of CV_AOSOMP_4_2d, see cv_solver.md beside it), and its algebra
is checked against numpy.linalg.solve of the same tridiagonal systems."""
import os

import numpy as np
import pytest

import cv_ref
import problems as pb
from test_capi_symbols import declared_symbols
from test_levelset import build_ls_stub
from test_mex_stubs import ROOT, call

F32 = np.float32
ENTRIES = ["pdeip_cv_solver", "pdeip_cv_solver_dev", "pdeip_cv_terms", "pdeip_cv_terms_dev"]
FIXTURE = os.path.join(ROOT, "tests", "golden", "levelset", "cv_solver.npz")


def fixture_cases():
    """[(name, PHI, D, DH, GradNorm, tau, nu, out)] of the golden file, arrays in MATLAB's column-major layout."""
    z = np.load(FIXTURE)
    cases = []
    for name in z["names"]:
        PHI, D, DH, G, out = (np.asfortranarray(z["%s/%s" % (name, k)]) for k in ("PHI", "D", "DH", "GradNorm", "out"))
        tau, nu = z["%s/tau_nu" % name]
        cases.append((str(name), PHI, D, DH, G, F32(tau), F32(nu), out))
    return cases


# ---- the restatement against the reference's outputs -------------------------------------------------------------------------

@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_restatement_matches_the_reference_bit_for_bit(case):
    name, PHI, D, DH, G, tau, nu, out = case
    got = cv_ref.CV_solver_2d(PHI, D, DH, G, tau, nu)
    assert pb.bit_equal(got, out), "%s: %s" % (name, pb.describe_mismatch(got, out))


def test_fixture_covers_the_cases_it_pins():
    cases = {c[0]: c for c in fixture_cases()}
    shapes = {c[1].shape for c in cases.values()}
    assert {(2, 2), (2, 9), (9, 2), (9, 13), (31, 17, 3), (40, 48, 3)} <= shapes
    assert len({(float(c[5]), float(c[6])) for c in cases.values()}) >= 3
    assert any(c[6] == 0 for c in cases.values())  # nu = 0
    _, PHI, D, DH, G, _, _, out = cases["nan12x10"]
    assert all(np.isnan(x).any() for x in (PHI, D, DH, G)) and np.isnan(out).any()
    G = cases["zeros9x13"][4]
    assert (G[0] == 0).any() and (G[-1] == 0).any() and (G[:, 0] == 0).any() and (G[:, -1] == 0).any()
    assert np.signbit(G[G == 0]).any()  # some -0.0
    assert (np.abs(cases["clamp31x17x3"][7]) == 5).sum() > 100
    assert os.path.getsize(FIXTURE) < 200 * 1024


# ---- the restatement on its own ----------------------------------------------------------------------------------------------

def _line_system(phi, d, dh, g, tau, nu):
    """float64 tridiagonal system of one line: w(p,q) = 2*tau*DH_p / (g_p + g_q), rhs PHI + tau*DH*D."""
    n = len(phi)
    phi, d, dh, g = (np.asarray(x, np.float64) for x in (phi, d, dh, g))

    def w(k, q):
        s = g[k] + g[q]
        return 2 * tau * dh[k] / s if s > 0 else 0.0

    A = np.zeros((n, n))
    for k in range(n):
        wn = w(k, k + 1) if k < n - 1 else 0.0
        wp = w(k, k - 1) if k > 0 else 0.0
        A[k, k] = 2 + nu * (wn + wp)
        if k > 0:
            A[k, k - 1] = -nu * wp
        if k < n - 1:
            A[k, k + 1] = -nu * wn
    return A, phi + tau * dh * d


def _problem(seed, shape, g_lo=0.2):
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-1, 1, shape).astype(F32)
    d = rng.uniform(-1, 1, shape).astype(F32)
    dh = rng.uniform(0.05, 0.3, shape).astype(F32)
    g = rng.uniform(g_lo, 2.0, shape).astype(F32)
    return [np.asfortranarray(x) for x in (phi, d, dh, g)]


@pytest.mark.parametrize("shape", [(2, 2), (3, 5), (17, 11), (9, 23, 2)])
def test_line_solves_solve_the_tridiagonal_systems(shape):
    phi, d, dh, g = _problem(3, shape)
    tau, nu = 0.25, 1.7
    xc = cv_ref.line_solve(phi, d, dh, g, tau, nu, 0)
    xr = cv_ref.line_solve(phi, d, dh, g, tau, nu, 1)
    p3, d3, h3, g3, c3, r3 = (x if x.ndim == 3 else x[:, :, None] for x in (phi, d, dh, g, xc, xr))
    for k in range(p3.shape[2]):
        for j in range(p3.shape[1]):
            A, rhs = _line_system(p3[:, j, k], d3[:, j, k], h3[:, j, k], g3[:, j, k], tau, nu)
            np.testing.assert_allclose(c3[:, j, k], np.linalg.solve(A, rhs), rtol=1e-5, atol=1e-5)
        for i in range(p3.shape[0]):
            A, rhs = _line_system(p3[i, :, k], d3[i, :, k], h3[i, :, k], g3[i, :, k], tau, nu)
            np.testing.assert_allclose(r3[i, :, k], np.linalg.solve(A, rhs), rtol=1e-5, atol=1e-5)
    # no zero gradient and nothing near +-5: the step is the plain sum of the two solves
    out = cv_ref.CV_solver_2d(phi, d, dh, g, tau, nu)
    assert np.abs(out).max() < 5
    assert np.array_equal(out, (F32(0) + xc) + xr)


def test_zero_gradient_rules():
    """A g == 0 pixel outside the first row and column takes clamp(PHI); in the first row (column pass never tests it) the
    row pass still does; in the first column the column pass does and the row pass adds its x; the (0, 0) pixel is never
    tested.  -0.0 counts as zero, NaN does not."""
    phi, d, dh, g = _problem(5, (6, 7))
    phi[2, 3], phi[0, 4], phi[3, 0] = F32(7.5), F32(-6), F32(1.25)
    for ij in ((2, 3), (0, 4), (3, 0), (0, 0)):
        g[ij] = 0
    g[4, 5] = F32(-0.0)
    g[1, 1] = np.nan
    tau, nu = F32(0.25), F32(1.0)
    out = cv_ref.CV_solver_2d(phi, d, dh, g, tau, nu)
    xc = cv_ref.line_solve(phi, d, dh, g, tau, nu, 0)
    xr = cv_ref.line_solve(phi, d, dh, g, tau, nu, 1)
    assert out[2, 3] == 5 and out[0, 4] == -5 and out[4, 5] == phi[4, 5]
    assert out[3, 0] == cv_ref.clamp(F32(1.25) + xr[3, 0])
    assert out[0, 0] == cv_ref.clamp(cv_ref.clamp(F32(0) + xc[0, 0]) + xr[0, 0])
    assert out[1, 1] == cv_ref.clamp(cv_ref.clamp(F32(0) + xc[1, 1]) + xr[1, 1])  # NaN != 0: the pixel keeps its solves


def test_clamp_lets_nan_through_and_turns_minus_zero_plus():
    v = np.array([np.nan, 6, -6, 5, -5, 4.5, -0.0], F32)
    c = cv_ref.clamp(v)
    assert np.isnan(c[0]) and list(c[1:6]) == [5, -5, 5, -5, 4.5] and np.signbit(c[6])
    phi, d, dh, g = _problem(6, (5, 4))
    phi[:] = F32(-0.0)
    d[:] = F32(-0.0)
    tau, nu = F32(0.25), F32(1)
    xc = cv_ref.line_solve(phi, d, dh, g, tau, nu, 0)
    xr = cv_ref.line_solve(phi, d, dh, g, tau, nu, 1)
    assert np.signbit(xc).all() and np.signbit(xr).all() and not (xc + xr != 0).any()
    out = cv_ref.CV_solver_2d(phi, d, dh, g, tau, nu)
    assert not np.signbit(out).any()  # 0.0f + x: the column value is +0.0, so the sum is too


def test_terms_follow_the_drivers_formulas():
    P = np.asfortranarray(np.array([[0, 1, np.nan], [-2, 3, 0.5]], F32))
    DH, G = cv_ref.cv_terms(P, 1, 1)
    assert DH[0, 0] == F32(1) / F32(np.pi) and np.isnan(DH[0, 2])
    DHf, _ = cv_ref.cv_terms(P, 1, 1, 0.06)
    assert DHf[1, 1] == F32(0.06) and np.isnan(DHf[0, 2])  # 1/(10 pi) < 0.06 is floored; NaN stays NaN
    DH2, _ = cv_ref.cv_terms(P, 2, 4, 0.04)
    assert DH2[1, 0] == F32(1) / (F32(np.pi) * F32(3))
    # replicate borders: central differences halve at the edges
    assert G[1, 1] == np.sqrt(F32((0.5 - -2) * 0.5) ** 2 + F32((3 - 1) * 0.5) ** 2)


# ---- the boundary ------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_cv_entries(pdeip):
    import ctypes

    syms = declared_symbols()
    lib = ctypes.CDLL(pdeip.capi.LIB_PATH)
    for name in ENTRIES:
        assert name in syms, name
        assert hasattr(lib, name), name
        assert name in pdeip.capi.SIGNATURES, name


def test_stub_checks_arity_types_sizes_and_outputs(pdeip):
    lib = build_ls_stub("CV_solver_2d", pdeip)
    z = np.zeros((5, 6), F32)
    good = [z, z, z, z, F32(0.25), F32(1)]
    err, _ = call(lib, 1, good[:5])
    assert err == "cv_solver_2D parameter error: wrong number of input parameters!"
    for k, name in enumerate(("PHI_in", "D_in", "DH_in", "GradNorm_in")):
        bad = list(good)
        bad[k] = z.astype(np.float64)
        err, _ = call(lib, 1, bad)
        assert err == "cv_solver_2D error: '%s' must be a noncomplex single-valued matrix." % name
    for k, name in ((4, "tau"), (5, "nu")):
        bad = list(good)
        bad[k] = np.float64(1)
        err, _ = call(lib, 1, bad)
        assert err == "cv_solver_2D error: '%s' must be a noncomplex, single-type scalar" % name
    for k in (1, 2, 3):
        bad = list(good)
        bad[k] = np.zeros((5, 5), F32)
        err, _ = call(lib, 1, bad)
        assert err == "cv_solver_2D error: 'D_in', 'DH_in' and 'GradNorm_in' must have the size of 'PHI_in'."
    err, _ = call(lib, 0, good)
    assert err == "cv_solver_2D error insufficient number of outputs. Outputs from this function is 'PHI_out'"
    err, _ = call(lib, 1, [np.zeros((1, 6), F32)] * 4 + good[4:])
    assert "at least 2x2" in err  # refused by the library before any HIP call


def test_mex_api_checks(pdeip):
    api = pdeip.mex_api
    z = np.zeros((5, 6), F32)
    with pytest.raises(api.MexError, match="cv_solver_2D error: 'DH_in' must be a noncomplex single-valued matrix"):
        api.CV_solver_2d(z, z, z.astype(np.float64), z, F32(0.25), F32(1))
    with pytest.raises(api.MexError, match="cv_solver_2D error: 'tau' must be a noncomplex, single-type scalar"):
        api.CV_solver_2d(z, z, z, z, 0.25, F32(1))
    with pytest.raises(api.MexError, match="'D_in', 'DH_in' and 'GradNorm_in' must have the size of 'PHI_in'"):
        api.CV_solver_2d(z, z, z, np.zeros((5, 7), F32), F32(0.25), F32(1))
    with pytest.raises(api.MexError, match="insufficient number of outputs"):
        api.CV_solver_2d(z, z, z, z, F32(0.25), F32(1), nargout=0)
    with pytest.raises(api.MexError, match="at least 2x2"):
        api.CV_solver_2d(*([np.zeros((6, 1), F32)] * 4), F32(0.25), F32(1))


@pytest.mark.parametrize("shape", [(1, 6), (6, 1), (1, 1)])
def test_c_abi_refuses_lines_shorter_than_two(pdeip, shape):
    capi = pdeip.capi
    lib = capi.load()
    z = np.zeros(shape, F32, order="F")
    o = np.zeros(shape, F32, order="F")
    p = z.ctypes.data
    rc = lib.pdeip_cv_solver(p, p, p, p, shape[0], shape[1], 1, 0.25, 1.0, o.ctypes.data)
    assert rc == capi.PDEIP_ERR_ARG and "at least 2x2" in capi.last_error()
    rc = lib.pdeip_cv_solver_dev(None, p, p, p, p, shape[0], shape[1], 1, 0.25, 1.0, o.ctypes.data)
    assert rc == capi.PDEIP_ERR_ARG and "at least 2x2" in capi.last_error()


def test_c_abi_refuses_aliases_and_empty_planes_without_a_gpu(pdeip):
    capi = pdeip.capi
    lib = capi.load()
    z = np.zeros((4, 4), F32, order="F")
    o = np.zeros((4, 4), F32, order="F")
    p, q = z.ctypes.data, o.ctypes.data
    assert lib.pdeip_cv_solver_dev(None, p, q, q, q, 4, 4, 1, 0.25, 1.0, q) == capi.PDEIP_ERR_ARG
    assert "alias" in capi.last_error()
    assert lib.pdeip_cv_terms(p, 4, 4, 1, 1.0, 1.0, 0.06, p, q) == capi.PDEIP_ERR_ARG and "alias" in capi.last_error()
    assert lib.pdeip_cv_terms_dev(None, p, 4, 4, 1, 1.0, 1.0, 0.06, q, q) == capi.PDEIP_ERR_ARG
    assert lib.pdeip_cv_terms(p, 0, 4, 1, 1.0, 1.0, 0.06, q, q) == capi.PDEIP_ERR_ARG and "empty" in capi.last_error()
