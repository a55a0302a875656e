"""NumPy restatement of what DispSegmentationSparse.m adds to the dense driver, as include/pdeip.h defines it: nanmedfilt2, the sparse
D pyramid, generateSeeds() / regionCompetition() with the pyramid builder and the starting gamma as arguments, and the sparse
driver (matlab/segmentation/DispSegmentationSparse.m:42-202, 679-685): the checker of pdeip_nanmedfilt2, pdeip_sparse_pyramid,
pdeip_generate_seeds_sparse, pdeip_region_competition_sparse and pdeip_disp_segmentation_sparse.

Independent of the product's kernels: the stages are segmentation_ref's, ransac_ref's, cv_ref's and ccl_ref's, imresize the
package's pyramid.py.  Arrays are MATLAB-shaped.  `perturb` and `trace` are the hooks of seeds_ref / segmentation_ref.  With
pyramid=plain_pyramid, gamma0=0.01 and the dense constants generate_seeds and the driver are seeds_ref's, bit for bit
(tests/test_sparse_ref.py)."""
import numpy as np

import ccl_ref
import cv_ref
import ransac_ref as rr
import seeds_ref as gs
import segmentation_ref as sr

F32 = np.float32
M64 = sr.M64
SEEDS_SPARSE = dict(gs.SPARSE)  # dist_cap 100, nan_fill 1000, mincov_gate 0.5
SEG_SPARSE = dict(sr.SPARSE)    # c0 2, c1 4, dh_floor 0.04, err_thr 1.2, gamma_coef 0.005, dist_cap 100, nan_fill 1000
GAMMA0_DENSE, GAMMA0_SPARSE = 0.01, 0.005
DRIVER = dict(srem_thr=0.002, polyorder=2, seeds=15, scl_factor=0.75, gen_scl=0.55, rc_scl=0.55, ransac_min_cset=0.1, ransac_max_cset=0.7,
              ransac_cset_cycles=10)


def nanmedfilt2(A):
    """The contract of pdeip_nanmedfilt2, step by step: the nine window values (0 outside the plane), sorted ascending with NaN
    last; n = the count of numbers; NaN for n == 0, else (float)(((double)v[(n-1)//2] + (double)v[n//2]) * 0.5) -- for odd n both
    are the (n+1)/2-th smallest and the expression returns it unchanged.  A [rows, cols] or [rows, cols, F]."""
    A = np.asarray(A, F32)
    if A.ndim == 3:
        return np.asfortranarray(np.stack([nanmedfilt2(A[:, :, f]) for f in range(A.shape[2])], axis=2))
    rows, cols = A.shape
    Z = np.zeros((rows + 2, cols + 2), F32)
    Z[1:-1, 1:-1] = A
    W = np.stack([Z[di:di + rows, dj:dj + cols] for dj in range(3) for di in range(3)], axis=0)  # [9, rows, cols]
    W = np.sort(W, axis=0)  # NaN last, as the kernel's exchange places it
    n = (~np.isnan(W)).sum(axis=0)
    lo = np.take_along_axis(W, np.maximum((n - 1) // 2, 0)[None], axis=0)[0]
    hi = np.take_along_axis(W, (n // 2)[None], axis=0)[0]
    with np.errstate(invalid="ignore"):
        med = ((lo.astype(np.float64) + hi.astype(np.float64)) * 0.5).astype(F32)
    return np.asfortranarray(np.where(n == 0, F32(np.nan), med).astype(F32))


def plain_pyramid(D, sz):
    """The dense drivers' D pyramid: cubic resizes."""
    py = sr._pyramid()
    P = [np.asarray(D, F32)]
    for r, c in sz[1:]:
        P.append(py.resize(P[-1], r, c, method="bicubic"))
    return P


def sparse_pyramid_sized(D, sz):
    """P_1 = nanmed(D), P_{k+1} = nanmed(resize_cubic(nanmed(P_k))) at the given sizes."""
    py = sr._pyramid()
    P = [nanmedfilt2(D)]
    for r, c in sz[1:]:
        P.append(nanmedfilt2(py.resize(nanmedfilt2(P[-1]), r, c, method="bicubic")))
    return P


def sparse_pyramid(D, scl_factor=0.75, pyr_scl=0.55):
    D = np.asarray(D, F32)
    return sparse_pyramid_sized(D, sr.scale_sizes(D.shape[0], D.shape[1], scl_factor, pyr_scl))


def generate_seeds(D, order, sigmaLim, cset_vect, iterations, AA=None, seeds=15, scl_factor=0.75, pyr_scl=0.55, seed=0, fit_counter=0, prm=None,
                   pyramid=sparse_pyramid_sized, gamma0=GAMMA0_SPARSE, defaults=None, perturb=None, trace=None):
    """generateSeeds() with the D pyramid's builder, the starting gamma and the constants' defaults as arguments.  Returns what
    seeds_ref.generate_seeds returns, plus Dp (the D pyramid)."""
    py = sr._pyramid()
    p = dict(SEEDS_SPARSE if defaults is None else defaults)
    p.update({k: v for k, v in (prm or {}).items() if not np.isnan(v)})
    D = np.asarray(D, F32)
    nrows, ncols = D.shape
    ncoef = 3 if order == 1 else 6
    sz = sr.scale_sizes(nrows, ncols, scl_factor, pyr_scl)
    K = len(sz)
    Dp = pyramid(D, sz)
    Df = [d if np.isnan(p["nan_fill"]) else np.where(np.isnan(d), F32(p["nan_fill"]), d).astype(F32) for d in Dp]
    AA1 = np.ones((nrows, ncols), F32) if AA is None else np.asarray(AA, F32).copy()
    AA1[np.isnan(AA1)] = 0
    gamma = float(gamma0)
    k = int(fit_counter)
    out_phi, out_surf = [], []
    for sd in range(seeds):
        Ap = [AA1]
        for r, c in sz[1:]:
            Ap.append(py.resize(Ap[-1], r, c, method="bicubic"))
        minCOV = float(sigmaLim)
        PHI = gs.initial_phi(nrows, ncols)
        empty = False
        M = None
        for v in range(2 * K):
            scl = gs.visit_scale(v, K)
            r, c = sz[scl]
            include = Ap[scl] > gs.INCLUDE_ABOVE
            min_aa = float(np.min(np.abs(Ap[scl].astype(np.float64) - float(gs.INCLUDE_ABOVE))))
            if v == 0:
                PHI = np.where(include, PHI, F32(-1)).astype(F32)
            M = None
            if v == K:
                _, _, areas = ccl_ref.label(PHI, 8)
                with np.errstate(invalid="ignore"):
                    min_phi = float(np.nanmin(np.abs(PHI)))
                PHI, _, _ = ccl_ref.largest_component(PHI, 8, 5.0, -5.0)
                if trace is not None:
                    trace.append(dict(seed=sd, visit=v, largest=PHI.copy(), areas=np.sort(np.asarray(areas))[::-1], min_phi=min_phi))
            nu = F32(gamma * (float(r) * float(c)) ** 0.7)
            last = None
            for it in range(1, iterations + 1):
                count = int(sr.sizes(PHI)[0])
                rec = dict(seed=sd, visit=v, iter=it, count=count, min_aa=min_aa, min_ransac=np.inf)
                with np.errstate(invalid="ignore"):
                    rec["min_phi"] = float(np.nanmin(np.abs(PHI)))
                if count < 20:
                    empty = True
                    if trace is not None:
                        trace.append(rec)
                    break
                res, M, dist, _ = rr.surface_fit_masked(PHI, Df[scl], order, M, 0.7, F32(gs.rcons(cset_vect, it, v)), gs.riter(it, v),
                                                        seed=(seed + 65536 * k) & M64)
                k += 1
                rec["min_ransac"] = sr._ransac_margin(res)
                cov, _ = sr.variance(PHI, dist, minCOV, p["dist_cap"])
                DH, G = cv_ref.cv_terms(PHI, 1.0, 1.0, np.nan)
                DH, G = DH.reshape(PHI.shape), G.reshape(PHI.shape)
                DATA = sr.data_term(dist, PHI, DH, cov, sr.INVERSE)["DATA"][:, :, 0]
                if perturb is not None:
                    DATA = perturb(DATA)
                DATA = np.where(include, DATA, F32(-2)).astype(F32)
                last = (PHI, dist)
                PHI = cv_ref.CV_solver_2d(PHI, DATA, DH, G, 1.0, nu).reshape(PHI.shape).astype(F32)
                rec["PHI"] = PHI.copy()
                if trace is not None:
                    trace.append(rec)
            if empty:
                gamma *= 0.8
                break
            if v == K and last is not None:
                var = float(sr.variance(last[0], last[1], -np.inf, p["dist_cap"])[0][0])
                if var > p["mincov_gate"]:
                    minCOV = var
            if v + 1 < 2 * K:
                rn, cn = sz[gs.visit_scale(v + 1, K)]
                PHI = py.resize(PHI, rn, cn, method="bicubic")
        if empty:
            continue
        out_phi.append(PHI)
        out_surf.append(np.asarray(M, F32) if M is not None else np.full(ncoef, np.nan, F32))
        AA1 = ((PHI < 0) & (AA1 != 0)).astype(F32)
    S = len(out_phi)
    PHIo = np.stack(out_phi, axis=2) if S else np.zeros((nrows, ncols, 0), F32)
    surf = np.stack(out_surf, axis=1) if S else np.zeros((ncoef, 0), F32)
    return dict(PHI=np.asfortranarray(PHIo), surf=surf, S=S, fit_counter=k, gamma=gamma, sizes=sz, Dp=Dp)


def region_competition(D, PHI, order, strategy, sigmaLim, ransac_cset, iterations, srem_thr, scl_factor=0.75, rc_scl=0.55, seed=0, prm=None,
                       pyramid=sparse_pyramid_sized, defaults=None, perturb=None, trace=None):
    """regionCompetition() with the D pyramid's builder and the constants' defaults as arguments: segmentation_ref.level per
    visit, PHI resized (bicubic) to the next visit's size."""
    py = sr._pyramid()
    p = dict(SEG_SPARSE if defaults is None else defaults)
    p.update({k: v for k, v in (prm or {}).items() if not np.isnan(v)})
    D = np.asarray(D, F32)
    PHI = sr._p3(PHI)
    sz = sr.scale_sizes(D.shape[0], D.shape[1], scl_factor, rc_scl)
    Dp = pyramid(D, sz)
    visits = list(range(len(sz))) + list(range(len(sz) - 1, -1, -1))
    kept = list(range(PHI.shape[2]))
    k = 0
    out = None
    for v, scl in enumerate(visits):
        tr = [] if trace is not None else None
        out = sr.level(PHI, Dp[scl], order, strategy, sigmaLim, ransac_cset, iterations, srem_thr, seed=seed, fit_counter=k, prm=p,
                       perturb=perturb, trace=tr)
        if trace is not None:
            for rec in tr:
                rec["visit"] = v
            trace.extend(tr)
        k = out["fit_counter"]
        kept = [kept[i] for i in out["kept"]]
        if out["S"] == 0:
            break
        PHI = out["PHI"]
        if v + 1 < len(visits):
            r, c = sz[visits[v + 1]]
            PHI = py.resize(PHI, r, c, method="bicubic")
    return dict(PHI=out["PHI"], surf=out["surf"], kept=kept, S=out["S"], fit_counter=k, sizes=sz, Dp=Dp)


def disp_segmentation_sparse(Din, PHI=None, AA=None, seed=0, perturb=None, trace=None, pyramid=sparse_pyramid_sized, gamma0=GAMMA0_SPARSE,
                             seeds_defaults=None, seg_defaults=None, driver_defaults=None, zero_nans=False, **param):
    """DispSegmentationSparse.m:42-202.  The keyword arguments after `trace` exist to tie this restatement to seeds_ref's dense
    driver: with plain_pyramid, 0.01, the dense constants, seeds_ref.DRIVER and zero_nans=True it is that driver.  Returns
    dict(PHI, SEG, surf, S, stages)."""
    p = dict(DRIVER if driver_defaults is None else driver_defaults)
    p.update(param)
    D = np.asarray(Din, F32).copy()
    if zero_nans:
        D[np.isnan(D)] = 0
    cset = gs.cset_vector(p["ransac_min_cset"], p["ransac_max_cset"], p["ransac_cset_cycles"])
    st = dict(j=0, PHI=np.zeros(D.shape + (0,), F32), surf=None)

    def stage_seed():
        s = (seed + (st["j"] << 32)) & M64
        st["j"] += 1
        return s

    def tr():
        return [] if trace is not None else None

    def keep(t, kind):
        if trace is not None:
            for rec in t:
                rec["stage"], rec["kind"] = st["j"] - 1, kind
            trace.extend(t)

    def compete(sigmaLim, iterations):
        t = tr()
        out = region_competition(D, st["PHI"], p["polyorder"], sr.INVERSE, sigmaLim, F32(p["ransac_max_cset"]), iterations, p["srem_thr"],
                                 scl_factor=p["scl_factor"], rc_scl=p["rc_scl"], seed=stage_seed(), pyramid=pyramid, defaults=seg_defaults,
                                 perturb=perturb, trace=t)
        keep(t, "rc")
        st["PHI"], st["surf"] = sr._p3(out["PHI"]), out["surf"]

    def more(sigmaLim, allowed, n, pyr_scl):
        t = tr()
        out = generate_seeds(D, p["polyorder"], sigmaLim, cset, 20, AA=allowed, seeds=n, scl_factor=p["scl_factor"], pyr_scl=pyr_scl,
                             seed=stage_seed(), pyramid=pyramid, gamma0=gamma0, defaults=seeds_defaults, perturb=perturb, trace=t)
        keep(t, "seeds")
        st["PHI"] = np.concatenate([st["PHI"], out["PHI"]], axis=2)
        st["surf"] = out["surf"] if st["surf"] is None else np.concatenate([st["surf"][:, :st["PHI"].shape[2] - out["S"]], out["surf"]], axis=1)

    def uncovered():
        return ((st["PHI"] > 0).sum(axis=2) == 0).astype(F32)

    def done():
        S = st["PHI"].shape[2]
        return dict(PHI=np.asfortranarray(st["PHI"]), SEG=sr.label(st["PHI"]) if S else None, surf=st["surf"], S=S, stages=st["j"])

    if PHI is None:
        more(0.7, None if AA is None else (np.asarray(AA) == 1).astype(F32), p["seeds"], p["gen_scl"])
        if st["PHI"].shape[2] and p["seeds"] != 1:
            compete(1.5, 30)
            if st["PHI"].shape[2]:
                more(1.2, uncovered(), p["seeds"], p["rc_scl"])
                compete(1.5, 20)
    else:
        st["PHI"] = sr._p3(PHI).copy()
        compete(1.0, 20)
        if st["PHI"].shape[2]:
            more(1.2, uncovered(), 1, p["rc_scl"])
            compete(2.0, 20)
    return done()
