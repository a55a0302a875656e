/* Iout = TVdenoisePD_gpu(I, u0, params)
 * Total-variation denoising by the first-order primal-dual iteration of Chambolle and Pock in one call, resident on the device
 * (pdeip_tv_pd, csrc/pdeip_tvpd.hip; the definition: include/pdeip.h).  Numeric arguments only; the wrapper matlab/TVdenoisePD_gpu.m
 * takes the name / value pairs and calls this:
 *   I        single or double [rows x cols (x frames)], NaN = no data (a double image is taken as single(I))
 *   u0       the start, of I's size, single or double; [] = I with its holes filled from the nearest known pixel
 *   params   real double vector [model lambda huber iter tau sigma]; model 0 = TV-L1, 1 = ROF (TV-L2); huber 0 = TV; tau, sigma NaN =
 *            the defaults 0.25 and 0.5
 *   Iout     single, the size of I
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

/* a whole number that fits an int */
static int is_count(double v)
{
    return v >= 0.0 && v <= 2147483647.0 && v == (double)(int)v;
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    pdeip_tvpd_params p;
    const double *pv;
    const float *I, *U0 = NULL;
    float *ownI = NULL, *ownU = NULL;
    size_t n;
    int rows, cols, F, rc, has_start;
    if (nrhs != 3) mexErrMsgTxt("TVdenoisePD_gpu parameter error: wrong number of input parameters!");
    if (nlhs != 1) mexErrMsgTxt("TVdenoisePD_gpu wrong number of outputs. The output of this function is 'Iout'");
    if (!is_field(prhs[0])) mexErrMsgTxt("TVdenoisePD_gpu: 'I' must be a noncomplex single or double array.");
    if (mxGetNumberOfDimensions(prhs[0]) > 3) mexErrMsgTxt("TVdenoisePD_gpu: 'I' must be a [rows x cols (x frames)] array");
    rows = pdeip_rows(prhs[0]);
    cols = pdeip_cols(prhs[0]);
    F = pdeip_frames(prhs[0]);
    if (rows < 1 || cols < 1 || F < 1) mexErrMsgTxt("TVdenoisePD_gpu: 'I' must be at least 1x1");
    has_start = mxGetNumberOfElements(prhs[1]) != 0;
    if (has_start) {
        if (!is_field(prhs[1])) mexErrMsgTxt("TVdenoisePD_gpu: 'u0' must be a noncomplex single or double array, or empty.");
        if (mxGetNumberOfDimensions(prhs[1]) > 3 || pdeip_rows(prhs[1]) != rows || pdeip_cols(prhs[1]) != cols || pdeip_frames(prhs[1]) != F)
            mexErrMsgTxt("TVdenoisePD_gpu: 'u0' must have the size of 'I'");
    }
    if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2]) || mxGetNumberOfElements(prhs[2]) != 6)
        mexErrMsgTxt("TVdenoisePD_gpu: 'params' must be a real double vector of 6 elements");
    pv = (const double *)mxGetData(prhs[2]);
    if (pv[0] != 0.0 && pv[0] != 1.0) mexErrMsgTxt("TVdenoisePD_gpu: 'model' must be 0 (TV-L1) or 1 (ROF)");
    if (!is_count(pv[3])) mexErrMsgTxt("TVdenoisePD_gpu: 'iter' must be a non-negative integer");
    p.model = pv[0] == 0.0 ? PDEIP_TVPD_L1 : PDEIP_TVPD_L2;
    p.lambda = pv[1];
    p.huber = pv[2];
    p.iter = (int)pv[3];
    p.tau = pv[4];
    p.sigma = pv[5];
    n = (size_t)rows * (size_t)cols * (size_t)F;
    I = as_single(prhs[0], n, &ownI);
    if (has_start) U0 = as_single(prhs[1], n, &ownU);
    if (I == NULL || (has_start && U0 == NULL)) {
        free(ownI);
        free(ownU);
        mexErrMsgTxt("TVdenoisePD_gpu: out of memory");
    }
    rc = pdeip_tv_pd(I, U0, rows, cols, F, &p, pdeip_out_like(&plhs[0], prhs[0]));
    free(ownI);
    free(ownU);
    pdeip_check(rc);
}
