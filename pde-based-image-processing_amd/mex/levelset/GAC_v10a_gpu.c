/* PHIout = GAC_v10a_gpu(Iin, PHIin, params)
 * The whole geodesic-active-contour driver matlab/active_contour/GAC_v10a.m in one call, resident on the device (pdeip_gac,
 * csrc/pdeip_levelset.hip).  Numeric arguments only; the wrapper matlab/GAC_v10a_gpu.m keeps the driver's argument list:
 *   Iin      single [rows x cols x channels]
 *   PHIin    single [rows x cols]
 *   params   double vector [tau c lambda ITER SMOOTH], NaN: the driver's default (lambda < 0: automatic) */
#include "../pdeip_mex_util.h"
#include "pdeip_gac_mex.h"

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    pdeip_gac_mex("GAC_v10a_gpu", PDEIP_GAC_A, nlhs, plhs, nrhs, prhs);
}
