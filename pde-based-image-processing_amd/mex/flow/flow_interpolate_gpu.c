/* [It, Ut, Vt, src] = flow_interpolate_gpu(I0, I1, Uf, Vf, Ub, Vb, t, params)
 * The frame at time t between two frames from a computed flow, in one call, resident on the device (pdeip_flow_interpolate,
 * csrc/pdeip_interp.hip; the definition: include/pdeip.h).  Numeric arguments only; the wrapper matlab/flow_interpolate_gpu.m takes
 * the name / value pairs and calls this:
 *   I0, I1   single or double [rows x cols (x channels)], the frames at t = 0 and t = 1 (a double array is taken as single(I))
 *   Uf, Vf   single or double [rows x cols], the flow of frame 0 -> 1
 *   Ub, Vb   the flow of frame 1 -> 0, or both [] for none (no occlusion reasoning)
 *   t        real double scalar, 0 < t < 1
 *   params   real double vector [a b use_costs alpha omega outer_iter inner_iter solver scl_factor min_size cover guide_scale keep]:
 *            a, b >= 0 the cross-checks' thresholds, use_costs 0 = the lowest index wins a pixel of the splat; the other ten are
 *            TVinpaint4_gpu's (<= 0 or NaN: the driver's default; guide_scale is not used)
 *   It       single, the size of I0
 *   Ut, Vt   single [rows x cols], the flow at t after the hole filling
 *   src      single [rows x cols]: 0 neither frame, 1 frame 0 alone, 2 frame 1 alone, 3 both blended
 * Every check below fires before anything touches the GPU. */
#include <stdlib.h>

#include "../pdeip_mex_util.h"

#define NPARAMS 13

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
    static const char *names[6] = {"I0", "I1", "Uf", "Vf", "Ub", "Vb"};
    pdeip_inpaint_params fill;
    pdeip_interp_params p;
    const double *pv, *f;
    const float *in[6] = {NULL, NULL, NULL, NULL, NULL, NULL};
    float *own[6] = {NULL, NULL, NULL, NULL, NULL, NULL}, *out[3] = {NULL, NULL, NULL};
    mwSize dims[2];
    size_t n, count;
    double t;
    int rows, cols, C, rc, k, has_back, failed = 0;
    if (nrhs != 8) mexErrMsgTxt("flow_interpolate_gpu parameter error: wrong number of input parameters!");
    if (nlhs < 1 || nlhs > 4)
        mexErrMsgTxt("flow_interpolate_gpu wrong number of outputs. Outputs from this function are 'It', 'Ut', 'Vt' and 'src'");
    has_back = mxGetNumberOfElements(prhs[4]) != 0;
    if (has_back != (mxGetNumberOfElements(prhs[5]) != 0)) mexErrMsgTxt("flow_interpolate_gpu: 'Ub' and 'Vb' must both be given or both be []");
    for (k = 0; k < (has_back ? 6 : 4); k++)
        if (!is_field(prhs[k])) {
            char msg[96];
            strcpy(msg, "flow_interpolate_gpu: '");
            strcat(msg, names[k]);
            strcat(msg, "' must be a noncomplex single or double array.");
            mexErrMsgTxt(msg);
        }
    if (mxGetNumberOfDimensions(prhs[0]) > 3) mexErrMsgTxt("flow_interpolate_gpu: 'I0' must be a [rows x cols (x channels)] array");
    rows = pdeip_rows(prhs[0]);
    cols = pdeip_cols(prhs[0]);
    C = pdeip_frames(prhs[0]);
    if (mxGetNumberOfDimensions(prhs[1]) > 3 || pdeip_rows(prhs[1]) != rows || pdeip_cols(prhs[1]) != cols || pdeip_frames(prhs[1]) != C)
        mexErrMsgTxt("flow_interpolate_gpu: 'I0' and 'I1' must have one size");
    for (k = 2; k < (has_back ? 6 : 4); k++)
        if (mxGetNumberOfDimensions(prhs[k]) != 2 || pdeip_rows(prhs[k]) != rows || pdeip_cols(prhs[k]) != cols)
            mexErrMsgTxt("flow_interpolate_gpu: the flow planes must be [rows x cols] arrays on the frame of 'I0'");
    if (!mxIsDouble(prhs[6]) || mxIsComplex(prhs[6]) || mxGetNumberOfElements(prhs[6]) != 1)
        mexErrMsgTxt("flow_interpolate_gpu: 't' must be a real double scalar");
    t = *(const double *)mxGetData(prhs[6]);
    if (!(t > 0.0 && t < 1.0)) mexErrMsgTxt("flow_interpolate_gpu: 't' must lie strictly between 0 and 1");
    if (!mxIsDouble(prhs[7]) || mxIsComplex(prhs[7]) || mxGetNumberOfElements(prhs[7]) != NPARAMS)
        mexErrMsgTxt("flow_interpolate_gpu: 'params' must be a real double vector of 13 elements");
    pv = (const double *)mxGetData(prhs[7]);
    f = pv + 3; /* TVinpaint4_gpu's ten */
    if (!(pv[0] >= 0.0) || !(pv[1] >= 0.0)) mexErrMsgTxt("flow_interpolate_gpu: 'a' and 'b' must be >= 0");
    for (k = 2; k < 7; k++) /* the integer members: outer_iter, inner_iter, solver, min_size */
        if (k != 5 && f[k] > 2147483647.0) mexErrMsgTxt("flow_interpolate_gpu: a parameter is too large");
    if (rows < 3 || cols < 3 || C < 1) mexErrMsgTxt("flow_interpolate_gpu: the frames must be at least 3x3");
    if (f[4] > 0.0 && f[4] != 1.0 && f[4] != 2.0) mexErrMsgTxt("flow_interpolate_gpu: 'solver' must be 1 (point SOR) or 2 (line relaxation)");
    if (f[5] >= 1.0) mexErrMsgTxt("flow_interpolate_gpu: 'scl_factor' must be below 1");
    if (f[7] > 1.0) mexErrMsgTxt("flow_interpolate_gpu: 'cover' must not be above 1");
    fill.alpha = f[0];
    fill.omega = f[1];
    fill.outer_iter = as_count(f[2]);
    fill.inner_iter = as_count(f[3]);
    fill.solver = as_count(f[4]);
    fill.scl_factor = f[5];
    fill.min_size = as_count(f[6]);
    fill.cover = f[7];
    fill.guide_scale = f[8];
    fill.keep = f[9] > 0.0 ? 1 : (f[9] == 0.0 ? 0 : -1);
    p.a = pv[0];
    p.b = pv[1];
    p.use_costs = pv[2] != 0.0;
    p.fill = &fill;
    n = (size_t)rows * (size_t)cols;
    for (k = 0; k < (has_back ? 6 : 4); k++) {
        count = k < 2 ? n * (size_t)C : n;
        in[k] = as_single(prhs[k], count, &own[k]);
        if (in[k] == NULL) failed = 1;
    }
    if (failed) {
        for (k = 0; k < 6; k++) free(own[k]);
        mexErrMsgTxt("flow_interpolate_gpu: out of memory");
    }
    plhs[0] = mxCreateNumericArray(mxGetNumberOfDimensions(prhs[0]), mxGetDimensions(prhs[0]), mxSINGLE_CLASS, mxREAL);
    dims[0] = (mwSize)rows;
    dims[1] = (mwSize)cols;
    for (k = 1; k < nlhs; k++) {
        plhs[k] = mxCreateNumericArray(2, dims, mxSINGLE_CLASS, mxREAL);
        out[k - 1] = (float *)mxGetData(plhs[k]);
    }
    rc = pdeip_flow_interpolate(in[0], in[1], C, in[2], in[3], in[4], in[5], rows, cols, t, &p, (float *)mxGetData(plhs[0]), out[0], out[1],
                                out[2]);
    for (k = 0; k < 6; k++) free(own[k]);
    pdeip_check(rc);
}
