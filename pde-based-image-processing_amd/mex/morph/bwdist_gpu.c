/* [D, IDX] = bwdist_gpu(BW)
 * [D, IDX] = bwdist(BW) with the Euclidean metric in one call on the device (pdeip_bwdist, csrc/pdeip_edt.hip; the definition:
 * include/pdeip.h).  Numeric arguments only; the wrapper matlab/bwdist_gpu.m converts a logical mask:
 *   BW    single or double [rows x cols]: the positive entries are the features (a double mask is taken as single(BW))
 *   D     single [rows x cols]: the distance to the nearest feature, Inf in a plane without one
 *   IDX   uint32 [rows x cols]: the 1-based linear index of that feature, as MATLAB's bwdist returns it; 0 where there is none.
 *         Among equidistant features the one with the lowest index wins.
 * Every check below fires before anything touches the GPU. */
#include <stdlib.h>

#include "../pdeip_mex_util.h"

/* mxUINT32_CLASS of MATLAB's matrix.h: the value is part of the MEX ABI (the mock runtime of the tests declares two classes only) */
#define BWDIST_UINT32_CLASS ((mxClassID)13)

static int is_plane(const mxArray *a)
{
    return (mxIsSingle(a) || mxIsDouble(a)) && !mxIsComplex(a);
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    const float *BW;
    float *own = NULL, *D;
    int *idx = NULL;
    unsigned int *IDX;
    size_t n, k;
    int rows, cols, rc;
    if (nrhs != 1) mexErrMsgTxt("bwdist_gpu parameter error: wrong number of input parameters!");
    if (nlhs < 1 || nlhs > 2) mexErrMsgTxt("bwdist_gpu wrong number of outputs. Outputs from this function are 'D' and 'IDX'");
    if (!is_plane(prhs[0])) mexErrMsgTxt("bwdist_gpu: 'BW' must be a noncomplex single or double array.");
    if (mxGetNumberOfDimensions(prhs[0]) != 2) mexErrMsgTxt("bwdist_gpu: 'BW' must be a [rows x cols] array");
    rows = pdeip_rows(prhs[0]);
    cols = pdeip_cols(prhs[0]);
    if (rows < 1 || cols < 1) mexErrMsgTxt("bwdist_gpu: 'BW' must be at least 1x1");
    n = (size_t)rows * (size_t)cols;
    if (mxIsDouble(prhs[0])) {
        const double *d = (const double *)mxGetData(prhs[0]);
        own = (float *)malloc(n * sizeof(float));
        if (own == NULL) mexErrMsgTxt("bwdist_gpu: out of memory");
        for (k = 0; k < n; k++) own[k] = (float)d[k];
        BW = own;
    } else {
        BW = (const float *)mxGetData(prhs[0]);
    }
    D = pdeip_out_like(&plhs[0], prhs[0]);
    if (nlhs > 1) {
        plhs[1] = mxCreateNumericArray(mxGetNumberOfDimensions(prhs[0]), mxGetDimensions(prhs[0]), BWDIST_UINT32_CLASS, mxREAL);
        idx = (int *)mxGetData(plhs[1]); /* the 0-based int32 index first, converted in place below */
    }
    rc = pdeip_bwdist(BW, rows, cols, 1, D, idx);
    free(own);
    pdeip_check(rc);
    if (idx != NULL) {
        IDX = (unsigned int *)mxGetData(plhs[1]);
        for (k = 0; k < n; k++) IDX[k] = idx[k] < 0 ? 0u : (unsigned int)idx[k] + 1u;
    }
}
