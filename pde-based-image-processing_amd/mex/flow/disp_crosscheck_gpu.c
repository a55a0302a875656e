/* [Ds, mask, stats] = disp_crosscheck_gpu(D0, D1, tol)
 * The left-right check of two disparities in one call on the device (pdeip_disp_crosscheck, csrc/pdeip_crosscheck.hip; the
 * definition: include/pdeip.h).  Numeric arguments only; the wrapper matlab/disp_crosscheck_gpu.m supplies the default:
 *   D0, D1   single or double [rows x cols], the checked view and the other view (a double map is taken as single(D))
 *   tol      real double scalar >= 0 (Inf allowed): the largest |D0 + D1(x + D0)| that is kept
 *   Ds       single [rows x cols]: D0 where kept, NaN elsewhere
 *   mask     single [rows x cols]: 1 where kept, 0 elsewhere
 *   stats    double [1 x 4]: kept, defined, mean and largest |D0 + D1(x + D0)| over the defined pixels
 * Every check below fires before anything touches the GPU. */
#include <stdlib.h>

#include "../pdeip_mex_util.h"

static int is_plane(const mxArray *a)
{
    return (mxIsSingle(a) || mxIsDouble(a)) && !mxIsComplex(a);
}

/* the plane as single: its own data, or a converted copy in *owned (to be freed) */
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
    const float *D0, *D1;
    float *own0 = NULL, *own1 = NULL, *mask = NULL;
    double *stats = NULL;
    double tol;
    mwSize sdims[2] = {1, 4};
    size_t n;
    int rows, cols, rc;
    if (nrhs != 3) mexErrMsgTxt("disp_crosscheck_gpu parameter error: wrong number of input parameters!");
    if (nlhs < 1 || nlhs > 3)
        mexErrMsgTxt("disp_crosscheck_gpu wrong number of outputs. Outputs from this function are 'Ds', 'mask' and 'stats'");
    if (!is_plane(prhs[0])) mexErrMsgTxt("disp_crosscheck_gpu: 'D0' must be a noncomplex single or double array.");
    if (!is_plane(prhs[1])) mexErrMsgTxt("disp_crosscheck_gpu: 'D1' must be a noncomplex single or double array.");
    if (mxGetNumberOfDimensions(prhs[0]) != 2 || mxGetNumberOfDimensions(prhs[1]) != 2 || pdeip_rows(prhs[0]) != pdeip_rows(prhs[1]) ||
        pdeip_cols(prhs[0]) != pdeip_cols(prhs[1]))
        mexErrMsgTxt("disp_crosscheck_gpu: 'D0' and 'D1' must be [rows x cols] arrays of one size");
    if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2]) || mxGetNumberOfElements(prhs[2]) != 1)
        mexErrMsgTxt("disp_crosscheck_gpu: 'tol' must be a real double scalar");
    tol = *(const double *)mxGetData(prhs[2]);
    if (!(tol >= 0.0)) mexErrMsgTxt("disp_crosscheck_gpu: 'tol' must be >= 0");
    rows = pdeip_rows(prhs[0]);
    cols = pdeip_cols(prhs[0]);
    if (rows < 1 || cols < 2) mexErrMsgTxt("disp_crosscheck_gpu: 'D0' must be at least 1x2");
    n = (size_t)rows * (size_t)cols;
    D0 = as_single(prhs[0], n, &own0);
    D1 = as_single(prhs[1], n, &own1);
    if (D0 == NULL || D1 == NULL) {
        free(own0);
        free(own1);
        mexErrMsgTxt("disp_crosscheck_gpu: out of memory");
    }
    if (nlhs > 1) mask = pdeip_out_like(&plhs[1], prhs[0]);
    if (nlhs > 2) {
        plhs[2] = mxCreateNumericArray(2, sdims, mxDOUBLE_CLASS, mxREAL);
        stats = (double *)mxGetData(plhs[2]);
    }
    rc = pdeip_disp_crosscheck(D0, D1, rows, cols, tol, pdeip_out_like(&plhs[0], prhs[0]), mask, NULL, stats);
    free(own0);
    free(own1);
    pdeip_check(rc);
}
