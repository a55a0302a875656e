/* [mask, err, stats] = flow_crosscheck_gpu(flowF, flowB, params)
 * The forward-backward check of two flows in one call on the device (pdeip_flow_crosscheck, csrc/pdeip_crosscheck.hip; the
 * definition: include/pdeip.h).  Numeric arguments only; the wrapper matlab/flow_crosscheck_gpu.m supplies the defaults:
 *   flowF    single or double [rows x cols x 2], cat(3, U, V) of frame 0 -> 1 (a double field is taken as single(flow))
 *   flowB    the same for frame 1 -> 0
 *   params   real double vector [a b], both >= 0 (Inf allowed): kept where |f + b(x+f)|^2 <= a (|f|^2 + |b(x+f)|^2) + b
 *   mask     single [rows x cols]: 1 where kept, 0 elsewhere
 *   err      single [rows x cols]: |f + b(x+f)|, NaN where x + f leaves the picture
 *   stats    double [1 x 4]: kept, defined, mean and largest err over the defined pixels
 * Every check below fires before anything touches the GPU. */
#include <stdlib.h>

#include "../pdeip_mex_util.h"

static int is_field(const mxArray *a)
{
    return (mxIsSingle(a) || mxIsDouble(a)) && !mxIsComplex(a);
}

/* the field as single: its own data, or a converted copy in *owned (to be freed) */
static const float *as_single(const mxArray *a, size_t n, float **owned)
{
    const double *d;
    size_t k;
    *owned = NULL;
    if (!mxIsDouble(a)) return (const float *)mxGetData(a);
    d = (const double *)mxGetData(a);
    *owned = (float *)malloc(n * sizeof(float));
    if (*owned == NULL) return NULL;
    for (k = 0; k < n; k++) (*owned)[k] = (float)d[k];
    return *owned;
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    const double *pv;
    const float *F, *B;
    float *ownF = NULL, *ownB = NULL, *err = NULL;
    double *stats = NULL;
    mwSize dims[2], sdims[2] = {1, 4};
    size_t n;
    int rows, cols, rc, k;
    if (nrhs != 3) mexErrMsgTxt("flow_crosscheck_gpu parameter error: wrong number of input parameters!");
    if (nlhs < 1 || nlhs > 3)
        mexErrMsgTxt("flow_crosscheck_gpu wrong number of outputs. Outputs from this function are 'mask', 'err' and 'stats'");
    if (!is_field(prhs[0])) mexErrMsgTxt("flow_crosscheck_gpu: 'flowF' must be a noncomplex single or double array.");
    if (!is_field(prhs[1])) mexErrMsgTxt("flow_crosscheck_gpu: 'flowB' must be a noncomplex single or double array.");
    for (k = 0; k < 2; k++)
        if (mxGetNumberOfDimensions(prhs[k]) != 3 || pdeip_frames(prhs[k]) != 2)
            mexErrMsgTxt("flow_crosscheck_gpu: 'flowF' and 'flowB' must be [rows x cols x 2] arrays");
    if (pdeip_rows(prhs[0]) != pdeip_rows(prhs[1]) || pdeip_cols(prhs[0]) != pdeip_cols(prhs[1]))
        mexErrMsgTxt("flow_crosscheck_gpu: 'flowF' and 'flowB' must have one size");
    if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2]) || mxGetNumberOfElements(prhs[2]) != 2)
        mexErrMsgTxt("flow_crosscheck_gpu: 'params' must be a real double vector of 2 elements");
    pv = (const double *)mxGetData(prhs[2]);
    if (!(pv[0] >= 0.0) || !(pv[1] >= 0.0)) mexErrMsgTxt("flow_crosscheck_gpu: 'a' and 'b' must be >= 0");
    rows = pdeip_rows(prhs[0]);
    cols = pdeip_cols(prhs[0]);
    if (rows < 2 || cols < 2) mexErrMsgTxt("flow_crosscheck_gpu: the flows must be at least 2x2x2");
    n = (size_t)rows * (size_t)cols;
    F = as_single(prhs[0], 2 * n, &ownF);
    B = as_single(prhs[1], 2 * n, &ownB);
    if (F == NULL || B == NULL) {
        free(ownF);
        free(ownB);
        mexErrMsgTxt("flow_crosscheck_gpu: out of memory");
    }
    dims[0] = (mwSize)rows;
    dims[1] = (mwSize)cols;
    plhs[0] = mxCreateNumericArray(2, dims, mxSINGLE_CLASS, mxREAL);
    if (nlhs > 1) {
        plhs[1] = mxCreateNumericArray(2, dims, mxSINGLE_CLASS, mxREAL);
        err = (float *)mxGetData(plhs[1]);
    }
    if (nlhs > 2) {
        plhs[2] = mxCreateNumericArray(2, sdims, mxDOUBLE_CLASS, mxREAL);
        stats = (double *)mxGetData(plhs[2]);
    }
    rc = pdeip_flow_crosscheck(F, F + n, B, B + n, rows, cols, pv[0], pv[1], (float *)mxGetData(plhs[0]), err, stats);
    free(ownF);
    free(ownB);
    pdeip_check(rc);
}
