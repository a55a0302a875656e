"""NumPy restatement of generateSeeds() and of the dense driver as include/pdeip.h defines them (matlab/segmentation/
DispSegmentation.m:31-198, 203-443): the checker of pdeip_generate_seeds and pdeip_disp_segmentation.

Independent of the product's kernels: the stages are segmentation_ref's, ransac_ref's, cv_ref's and ccl_ref's, imresize the
package's pyramid.py.  Arrays are MATLAB-shaped.  `perturb` and `trace` are the hooks of segmentation_ref.level: perturb moves
DATA, trace (a list) receives one dict per iteration (seed, visit, iter, count, min_phi, min_ransac, min_aa, PHI after the step)
and one per v = K visit (seed, visit, largest: the selected plane, areas: the component areas of the plane before the selection
in descending order, min_phi: that plane's smallest |PHI|)."""
import numpy as np

import ccl_ref
import cv_ref
import ransac_ref as rr
import segmentation_ref as sr

F32 = np.float32
M64 = sr.M64
DENSE = dict(dist_cap=np.inf, nan_fill=np.nan, mincov_gate=-np.inf)
SPARSE = dict(dist_cap=100.0, nan_fill=1000.0, mincov_gate=0.5)
INCLUDE_ABOVE = F32(0.05)


def initial_phi(nrows, ncols):
    P = -np.ones((nrows, ncols), F32)
    P[1:nrows - 1:5, 1:ncols - 1:5] = 1  # PHIinitial(2:5:end-1, 2:5:end-1) = 1
    return P


def visit_scale(v, K):
    return v if v < K else 2 * K - 1 - v


def riter(it, v):
    return 2000 if it <= 1 and v == 0 else 100


def rcons(cset_vect, it, v):
    return cset_vect[-1] if v != 0 else cset_vect[min(it, len(cset_vect)) - 1]


def generate_seeds(D, order, sigmaLim, cset_vect, iterations, AA=None, seeds=15, scl_factor=0.7, pyr_scl=0.2, seed=0, fit_counter=0,
                   prm=None, perturb=None, trace=None):
    """Returns dict(PHI [nrows, ncols, S], surf [ncoef, S], S, fit_counter, gamma, sizes)."""
    py = sr._pyramid()
    p = dict(DENSE)
    p.update(prm or {})
    D = np.asarray(D, F32)
    nrows, ncols = D.shape
    ncoef = 3 if order == 1 else 6
    sz = sr.scale_sizes(nrows, ncols, scl_factor, pyr_scl)
    K = len(sz)
    Dp = [D]
    for r, c in sz[1:]:
        Dp.append(py.resize(Dp[-1], r, c, method="bicubic"))
    Df = [d if np.isnan(p["nan_fill"]) else np.where(np.isnan(d), F32(p["nan_fill"]), d).astype(F32) for d in Dp]
    AA1 = np.ones((nrows, ncols), F32) if AA is None else np.asarray(AA, F32).copy()
    AA1[np.isnan(AA1)] = 0
    gamma = 0.01
    k = int(fit_counter)
    out_phi, out_surf = [], []
    for sd in range(seeds):
        Ap = [AA1]
        for r, c in sz[1:]:
            Ap.append(py.resize(Ap[-1], r, c, method="bicubic"))
        minCOV = float(sigmaLim)
        PHI = initial_phi(nrows, ncols)
        empty = False
        M = None
        for v in range(2 * K):
            scl = visit_scale(v, K)
            r, c = sz[scl]
            include = Ap[scl] > INCLUDE_ABOVE
            min_aa = float(np.min(np.abs(Ap[scl].astype(np.float64) - float(INCLUDE_ABOVE))))
            if v == 0:
                PHI = np.where(include, PHI, F32(-1)).astype(F32)
            M = None
            if v == K:
                _, _, areas = ccl_ref.label(PHI, 8)  # of the plane the selection is made on
                with np.errstate(invalid="ignore"):
                    min_phi = float(np.nanmin(np.abs(PHI)))  # the `> 0` of bwlabel(PHI > 0)
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
                res, M, dist, _ = rr.surface_fit_masked(PHI, Df[scl], order, M, 0.7, F32(rcons(cset_vect, it, v)), riter(it, v),
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
                rn, cn = sz[visit_scale(v + 1, K)]
                PHI = py.resize(PHI, rn, cn, method="bicubic")
        if empty:
            continue
        out_phi.append(PHI)
        out_surf.append(np.asarray(M, F32) if M is not None else np.full(ncoef, np.nan, F32))  # iterations == 0: no model
        AA1 = ((PHI < 0) & (AA1 != 0)).astype(F32)
    S = len(out_phi)
    PHIo = np.stack(out_phi, axis=2) if S else np.zeros((nrows, ncols, 0), F32)
    surf = np.stack(out_surf, axis=1) if S else np.zeros((ncoef, 0), F32)
    return dict(PHI=np.asfortranarray(PHIo), surf=surf, S=S, fit_counter=k, gamma=gamma, sizes=sz)


DRIVER = dict(srem_thr=0.002, polyorder=1, seeds=15, scl_factor=0.7, gen_scl=0.2, rc_scl=0.4, ransac_min_cset=0.1, ransac_max_cset=0.7,
              ransac_cset_cycles=10)


def cset_vector(lo, hi, cycles):
    step = (hi - lo) / cycles
    return [lo + step * float(i) for i in range(cycles + 1)]


def disp_segmentation(Din, PHI=None, AA=None, seed=0, perturb=None, trace=None, **param):
    """Returns dict(PHI, SEG, surf, S, stages: the number of stage calls made)."""
    p = dict(DRIVER)
    p.update(param)
    D = np.asarray(Din, F32).copy()
    D[np.isnan(D)] = 0
    cset = cset_vector(p["ransac_min_cset"], p["ransac_max_cset"], p["ransac_cset_cycles"])
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
        out = sr.region_competition(D, st["PHI"], p["polyorder"], sr.INVERSE, sigmaLim, F32(p["ransac_max_cset"]), iterations, p["srem_thr"],
                                    scl_factor=p["scl_factor"], rc_scl=p["rc_scl"], seed=stage_seed(), perturb=perturb, trace=t)
        keep(t, "rc")
        st["PHI"], st["surf"] = sr._p3(out["PHI"]), out["surf"]

    def more(sigmaLim, allowed, n, pyr_scl):
        t = tr()
        out = generate_seeds(D, p["polyorder"], sigmaLim, cset, 20, AA=allowed, seeds=n, scl_factor=p["scl_factor"], pyr_scl=pyr_scl,
                             seed=stage_seed(), perturb=perturb, trace=t)
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
