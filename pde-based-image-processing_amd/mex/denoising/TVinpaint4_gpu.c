/* [Dout, filled] = TVinpaint4_gpu(D, guide, params)
 * The holes (NaN) of a sparse disparity or flow map filled by total-variation inpainting in one call, resident on the device
 * (pdeip_tv_inpaint4, csrc/pdeip_inpaint.hip; the definition: include/pdeip.h).  Numeric arguments only; the wrapper
 * matlab/TVinpaint4_gpu.m takes the name / value pairs and calls this:
 *   D        single or double [rows x cols (x frames)], NaN = no estimate (a double map is taken as single(D)); a flow is cat(3, U, V)
 *   guide    single or double [rows x cols (x channels)] on D's frame, or [] for none
 *   params   real double vector [alpha omega outer_iter inner_iter solver scl_factor min_size cover guide_scale keep]; <= 0 or NaN:
 *            the driver's default (5, 1.75, 10, 5, 2, 0.75, 16, 0.25, 20); keep: 0 = the solver's values everywhere, > 0 = known
 *            pixels keep their own bits, < 0 or NaN = the default (keep)
 *   Dout     single, the size of D, no NaN left
 *   filled   single, the size of D: 1 where D was a hole, 0 elsewhere
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

/* an integer member: <= 0 or NaN is 0 (the default); anything beyond int's range is refused by the caller */
static int as_count(double v)
{
    return v > 0.0 ? (int)v : 0;
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    pdeip_inpaint_params p;
    const double *pv;
    const float *D, *G = NULL;
    float *ownD = NULL, *ownG = NULL, *filled = NULL;
    size_t n;
    int rows, cols, F, C = 0, rc, k, has_guide;
    if (nrhs != 3) mexErrMsgTxt("TVinpaint4_gpu parameter error: wrong number of input parameters!");
    if (nlhs < 1 || nlhs > 2) mexErrMsgTxt("TVinpaint4_gpu wrong number of outputs. Outputs from this function are 'Dout' and 'filled'");
    if (!is_field(prhs[0])) mexErrMsgTxt("TVinpaint4_gpu: 'D' must be a noncomplex single or double array.");
    if (mxGetNumberOfDimensions(prhs[0]) > 3) mexErrMsgTxt("TVinpaint4_gpu: 'D' must be a [rows x cols (x frames)] array");
    rows = pdeip_rows(prhs[0]);
    cols = pdeip_cols(prhs[0]);
    F = pdeip_frames(prhs[0]);
    has_guide = mxGetNumberOfElements(prhs[1]) != 0;
    if (has_guide) {
        if (!is_field(prhs[1])) mexErrMsgTxt("TVinpaint4_gpu: 'guide' must be a noncomplex single or double array, or empty.");
        if (mxGetNumberOfDimensions(prhs[1]) > 3 || pdeip_rows(prhs[1]) != rows || pdeip_cols(prhs[1]) != cols)
            mexErrMsgTxt("TVinpaint4_gpu: 'guide' must be a [rows x cols (x channels)] array on the frame of 'D'");
        C = pdeip_frames(prhs[1]);
    }
    if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2]) || mxGetNumberOfElements(prhs[2]) != 10)
        mexErrMsgTxt("TVinpaint4_gpu: 'params' must be a real double vector of 10 elements");
    pv = (const double *)mxGetData(prhs[2]);
    for (k = 2; k < 7; k++) /* the integer members: outer_iter, inner_iter, solver, min_size */
        if (k != 5 && pv[k] > 2147483647.0) mexErrMsgTxt("TVinpaint4_gpu: a parameter is too large");
    if (rows < 3 || cols < 3 || F < 1) mexErrMsgTxt("TVinpaint4_gpu: 'D' must be at least 3x3");
    if (pv[4] > 0.0 && pv[4] != 1.0 && pv[4] != 2.0) mexErrMsgTxt("TVinpaint4_gpu: 'solver' must be 1 (point SOR) or 2 (line relaxation)");
    if (pv[5] >= 1.0) mexErrMsgTxt("TVinpaint4_gpu: 'scl_factor' must be below 1");
    if (pv[7] > 1.0) mexErrMsgTxt("TVinpaint4_gpu: 'cover' must not be above 1");
    p.alpha = pv[0];
    p.omega = pv[1];
    p.outer_iter = as_count(pv[2]);
    p.inner_iter = as_count(pv[3]);
    p.solver = as_count(pv[4]);
    p.scl_factor = pv[5];
    p.min_size = as_count(pv[6]);
    p.cover = pv[7];
    p.guide_scale = pv[8];
    p.keep = pv[9] > 0.0 ? 1 : (pv[9] == 0.0 ? 0 : -1);
    n = (size_t)rows * (size_t)cols;
    D = as_single(prhs[0], n * (size_t)F, &ownD);
    if (has_guide) G = as_single(prhs[1], n * (size_t)C, &ownG);
    if (D == NULL || (has_guide && G == NULL)) {
        free(ownD);
        free(ownG);
        mexErrMsgTxt("TVinpaint4_gpu: out of memory");
    }
    plhs[0] = mxCreateNumericArray(mxGetNumberOfDimensions(prhs[0]), mxGetDimensions(prhs[0]), mxSINGLE_CLASS, mxREAL);
    if (nlhs > 1) {
        plhs[1] = mxCreateNumericArray(mxGetNumberOfDimensions(prhs[0]), mxGetDimensions(prhs[0]), mxSINGLE_CLASS, mxREAL);
        filled = (float *)mxGetData(plhs[1]);
    }
    rc = pdeip_tv_inpaint4(D, rows, cols, F, G, C, &p, (float *)mxGetData(plhs[0]), filled);
    free(ownD);
    free(ownG);
    pdeip_check(rc);
}
