/* PHI_out = Reinit(PHI_in, T)
 * Drop-in for mex/source/Reinit.c (reference gateway :47-139): the re-initialisation steps of t = 0:0.25:T.  Unlike the
 * reference, which re-initialises PHI_in in place before copying it out (:136-137), PHI_in is left unchanged. */
#include "../pdeip_mex_util.h"

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    const float *PHI;
    float T, *out;
    if (nrhs != 2) mexErrMsgTxt("reInitC parameter error: wrong number of input parameters!");
    PHI = pdeip_single(prhs[0], "reInitC", "PHI_in");
    T = pdeip_scalar(prhs[1], "reInitC error", "T");
    if (nlhs < 1) mexErrMsgTxt("reInitC error insufficient number of outputs. Outputs from this function is 'PHI_out'");
    out = pdeip_out_like(&plhs[0], prhs[0]);
    pdeip_check(pdeip_reinit(PHI, pdeip_rows(prhs[0]), pdeip_cols(prhs[0]), pdeip_frames(prhs[0]), T, out));
}
