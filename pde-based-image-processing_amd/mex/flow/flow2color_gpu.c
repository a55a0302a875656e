/* [img, maxvalue] = flow2color_gpu(flow, params)
 * The colour coding matlab/optical_flow/flow2color.m in one call on the device (pdeip_flow2color, csrc/pdeip_flowviz.hip).  Numeric
 * arguments only; the wrapper matlab/flow2color_gpu.m keeps the function's argument list:
 *   flow       single or double [rows x cols x 2] (a double field is taken as single(flow))
 *   params     real double vector [maxvalue border]; maxvalue NaN: the field's largest magnitude; border a non-negative integer
 *   img        single [rows + 2 border x cols + 2 border x 3]
 *   maxvalue   double scalar, the maximum used (what the .m displays)
 * Every check below fires before anything touches the GPU. */
#include <stdlib.h>

#include "../pdeip_mex_util.h"

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    const double *pv;
    const float *U;
    float *tmp = NULL, *img;
    double *used;
    mwSize dims[3], one[2] = {1, 1};
    size_t n, k;
    int rows, cols, border, rc;
    if (nrhs != 2) mexErrMsgTxt("flow2color_gpu parameter error: wrong number of input parameters!");
    if (nlhs < 1) mexErrMsgTxt("flow2color_gpu insufficient number of outputs. Outputs from this function are 'img' and 'maxvalue'");
    if ((!mxIsSingle(prhs[0]) && !mxIsDouble(prhs[0])) || mxIsComplex(prhs[0]))
        mexErrMsgTxt("flow2color_gpu: 'flow' must be a noncomplex single or double array.");
    if (mxGetNumberOfDimensions(prhs[0]) != 3 || pdeip_frames(prhs[0]) != 2)
        mexErrMsgTxt("flow2color_gpu: 'flow' must be a [rows x cols x 2] array");
    if (!mxIsDouble(prhs[1]) || mxIsComplex(prhs[1]) || mxGetNumberOfElements(prhs[1]) != 2)
        mexErrMsgTxt("flow2color_gpu: 'params' must be a real double vector of 2 elements");
    pv = (const double *)mxGetData(prhs[1]);
    if (!(pv[1] >= 0.0) || pv[1] > 1073741823.0 || pv[1] != (double)(int)pv[1])
        mexErrMsgTxt("flow2color_gpu: 'border' must be a non-negative integer");
    border = (int)pv[1];
    rows = pdeip_rows(prhs[0]);
    cols = pdeip_cols(prhs[0]);
    if (rows < 1 || cols < 1) mexErrMsgTxt("flow2color_gpu: 'flow' must be at least 1x1x2");
    n = (size_t)rows * (size_t)cols;
    dims[0] = (mwSize)rows + 2 * (mwSize)border;
    dims[1] = (mwSize)cols + 2 * (mwSize)border;
    dims[2] = 3;
    if (mxIsDouble(prhs[0])) {
        const double *d = (const double *)mxGetData(prhs[0]);
        tmp = (float *)malloc(2 * n * sizeof(float));
        if (tmp == NULL) mexErrMsgTxt("flow2color_gpu: out of memory");
        for (k = 0; k < 2 * n; k++) tmp[k] = (float)d[k];
        U = tmp;
    } else {
        U = (const float *)mxGetData(prhs[0]);
    }
    plhs[0] = mxCreateNumericArray(3, dims, mxSINGLE_CLASS, mxREAL);
    img = (float *)mxGetData(plhs[0]);
    if (nlhs > 1) {
        plhs[1] = mxCreateNumericArray(2, one, mxDOUBLE_CLASS, mxREAL);
        used = (double *)mxGetData(plhs[1]);
    } else {
        used = NULL;
    }
    rc = pdeip_flow2color(U, U + n, rows, cols, pv[0], border, img, NULL, used);
    free(tmp);
    pdeip_check(rc);
}
