/* Iout = Diffusion8_gpu(I, params)
 * Structure-tensor anisotropic diffusion (Weickert's edge-enhancing and coherence-enhancing diffusion) in one call, resident on the
 * device (pdeip_diffusion8, csrc/pdeip_stensor.hip).  Numeric arguments only; the wrapper matlab/Diffusion8_gpu.m takes the mode by
 * name and name-value parameters and applies the uint8 cast:
 *   I        single [rows x cols x C]
 *   params   real double vector [mode sigma rho lambda alpha C tau iters inner_iter omega solver], mode 0 = EED, 1 = CED; NaN: the
 *            default of the mode (include/pdeip.h)
 *   Iout     single [rows x cols x C], the result before the cast */
#include "../pdeip_mex_util.h"

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    static const char *who = "Diffusion8_gpu";
    pdeip_diffusion8_params p;
    const float *I;
    const double *pv;
    float *out;
    if (nrhs != 2) mexErrMsgTxt("Diffusion8_gpu parameter error: wrong number of input parameters!");
    if (nlhs < 1) mexErrMsgTxt("Diffusion8_gpu insufficient number of outputs. Output from this function is 'Iout'");
    I = pdeip_single(prhs[0], who, "I");
    if (mxGetNumberOfDimensions(prhs[0]) > 3) mexErrMsgTxt("Diffusion8_gpu: 'I' must be a [rows x cols x C] array");
    if (!mxIsDouble(prhs[1]) || mxIsComplex(prhs[1]) || mxGetNumberOfElements(prhs[1]) != 11)
        mexErrMsgTxt("Diffusion8_gpu: 'params' must be a real double vector of 11 elements");
    pv = (const double *)mxGetData(prhs[1]);
    p.mode = pv[0];
    p.sigma = pv[1];
    p.rho = pv[2];
    p.lambda = pv[3];
    p.alpha = pv[4];
    p.C = pv[5];
    p.tau = pv[6];
    p.iters = pv[7];
    p.inner_iter = pv[8];
    p.omega = pv[9];
    p.solver = pv[10];
    out = pdeip_out_like(&plhs[0], prhs[0]);
    pdeip_check(pdeip_diffusion8(I, pdeip_rows(prhs[0]), pdeip_cols(prhs[0]), pdeip_frames(prhs[0]), &p, out));
}
