/* Iout = Diffusion4_v10_gpu(I, params)
 * The nonlinear diffusion filter matlab/diffusion/Diffusion4_v10.m in one call, resident on the device (pdeip_diffusion4,
 * csrc/pdeip_diffusion.hip).  Numeric arguments only; the wrapper matlab/Diffusion4_v10_gpu.m keeps the driver's argument list
 * and applies its uint8 cast:
 *   I        single [rows x cols x C]
 *   params   real double vector [alpha outer_iter], NaN: the driver's default (25, 5)
 *   Iout     single [rows x cols x C], the result before the cast */
#include "../pdeip_mex_util.h"

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    static const char *who = "Diffusion4_v10_gpu";
    pdeip_diffusion4_params p;
    const float *I;
    const double *pv;
    float *out;
    if (nrhs != 2) mexErrMsgTxt("Diffusion4_v10_gpu parameter error: wrong number of input parameters!");
    if (nlhs < 1) mexErrMsgTxt("Diffusion4_v10_gpu insufficient number of outputs. Output from this function is 'Iout'");
    I = pdeip_single(prhs[0], who, "I");
    if (mxGetNumberOfDimensions(prhs[0]) > 3) mexErrMsgTxt("Diffusion4_v10_gpu: 'I' must be a [rows x cols x C] array");
    if (!mxIsDouble(prhs[1]) || mxIsComplex(prhs[1]) || mxGetNumberOfElements(prhs[1]) != 2)
        mexErrMsgTxt("Diffusion4_v10_gpu: 'params' must be a real double vector of 2 elements");
    pv = (const double *)mxGetData(prhs[1]);
    p.alpha = pv[0];
    p.outer_iter = pv[1];
    out = pdeip_out_like(&plhs[0], prhs[0]);
    pdeip_check(pdeip_diffusion4(I, pdeip_rows(prhs[0]), pdeip_cols(prhs[0]), pdeip_frames(prhs[0]), &p, out));
}
