"""NumPy restatement of pdeip_surface_fit_masked_batch_dev as include/pdeip.h defines it: the loop over
ransac_ref.surface_fit_masked with the per-segment seed, and nothing else."""
import numpy as np

import ransac_ref as ref

F32 = np.float32


def surface_fit_masked_batch(PHI, D, order, M_in, err_thr, min_set_size, iter, seed=0, seed_stride=65536):
    """surface_fit_masked of every plane PHI[:, :, s] over the one data plane D, segment s drawing from seed + seed_stride*s (64-bit
    wrapping); M_in [ncoef, S] or None.  Returns (list of result dicts, M_out [ncoef, S], dist [nrows, ncols, S], ndata int [S])."""
    PHI = np.asarray(PHI)
    S = PHI.shape[2]
    res, M, dist, ndata = [], [], [], []
    for s in range(S):
        given = None if M_in is None else np.asarray(M_in, F32)[:, s]
        r, m, d, n = ref.surface_fit_masked(PHI[:, :, s], D, order, given, err_thr, min_set_size, iter, seed=(seed + seed_stride * s) & ref.M64)
        res.append(r)
        M.append(m)
        dist.append(d)
        ndata.append(n)
    return res, np.stack(M, axis=1), np.asfortranarray(np.stack(dist, axis=2)), np.array(ndata, np.int64)
