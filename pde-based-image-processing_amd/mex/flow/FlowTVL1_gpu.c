/* [U, V] = FlowTVL1_gpu(Iin, params)
 * TV-L1 optical flow in one call, resident on the device: Zach, Pock and Bischof's model by the first-order primal-dual iteration of
 * Chambolle and Pock, warped and coarse to fine (pdeip_flow_tvl1, csrc/pdeip_drivers.hip and csrc/pdeip_tvl1.hip; the definition:
 * include/pdeip.h).  Numeric arguments only; the wrapper matlab/FlowTVL1_gpu.m takes the name / value pairs and calls this:
 *   Iin      single or double [rows x cols x 2], gray, 0..255: cat(3, frame0, frame1) (a double pair is taken as single(Iin))
 *   params   real double vector [lambda huber tau sigma scl_factor warps iter scales]; a member that is <= 0 or NaN keeps the
 *            driver's default (15, 0, 0.25, 0.5, 0.75, 3, 20, all scales)
 *   U, V     single [rows x cols]: the flow along the columns and down the rows
 * Every check below fires before anything touches the GPU. */
#include <stdlib.h>

#include "../pdeip_mex_util.h"

/* a count the driver takes: a whole number that fits an int, or "<= 0 or NaN: the default" as 0 */
static int as_count(double v, int *out)
{
    if (!(v > 0.0)) {
        *out = 0;
        return 1;
    }
    if (v > 2147483647.0 || v != (double)(int)v) return 0;
    *out = (int)v;
    return 1;
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    pdeip_flow_tvl1_params p;
    const double *pv;
    const float *I;
    float *own = NULL, *U, *V;
    mwSize dims[2];
    size_t n, k;
    int rows, cols, rc;
    if (nrhs != 2) mexErrMsgTxt("FlowTVL1_gpu parameter error: wrong number of input parameters!");
    if (nlhs != 2) mexErrMsgTxt("FlowTVL1_gpu wrong number of outputs. The outputs of this function are 'U' and 'V'");
    if (!(mxIsSingle(prhs[0]) || mxIsDouble(prhs[0])) || mxIsComplex(prhs[0])) mexErrMsgTxt("FlowTVL1_gpu: 'Iin' must be a noncomplex single or double array.");
    if (mxGetNumberOfDimensions(prhs[0]) != 3 || pdeip_frames(prhs[0]) != 2) mexErrMsgTxt("FlowTVL1_gpu: 'Iin' must be a [rows x cols x 2] array");
    rows = pdeip_rows(prhs[0]);
    cols = pdeip_cols(prhs[0]);
    if (rows < 2 || cols < 2) mexErrMsgTxt("FlowTVL1_gpu: the frames must be at least 2x2");
    if (!mxIsDouble(prhs[1]) || mxIsComplex(prhs[1]) || mxGetNumberOfElements(prhs[1]) != 8)
        mexErrMsgTxt("FlowTVL1_gpu: 'params' must be a real double vector of 8 elements");
    pv = (const double *)mxGetData(prhs[1]);
    p.lambda = pv[0];
    p.huber = pv[1];
    p.tau = pv[2];
    p.sigma = pv[3];
    p.scl_factor = pv[4];
    if (!as_count(pv[5], &p.warps)) mexErrMsgTxt("FlowTVL1_gpu: 'warps' must be a whole number");
    if (!as_count(pv[6], &p.iter)) mexErrMsgTxt("FlowTVL1_gpu: 'iter' must be a whole number");
    if (!as_count(pv[7], &p.scales)) mexErrMsgTxt("FlowTVL1_gpu: 'scales' must be a whole number");
    n = (size_t)rows * (size_t)cols * 2;
    if (mxIsDouble(prhs[0])) {
        const double *d = (const double *)mxGetData(prhs[0]);
        own = (float *)malloc(n * sizeof(float));
        if (own == NULL) mexErrMsgTxt("FlowTVL1_gpu: out of memory");
        for (k = 0; k < n; k++) own[k] = (float)d[k];
        I = own;
    } else {
        I = (const float *)mxGetData(prhs[0]);
    }
    dims[0] = (mwSize)rows;
    dims[1] = (mwSize)cols;
    plhs[0] = mxCreateNumericArray(2, dims, mxSINGLE_CLASS, mxREAL);
    plhs[1] = mxCreateNumericArray(2, dims, mxSINGLE_CLASS, mxREAL);
    U = (float *)mxGetData(plhs[0]);
    V = (float *)mxGetData(plhs[1]);
    rc = pdeip_flow_tvl1(I, rows, cols, &p, U, V);
    free(own);
    pdeip_check(rc);
}
