/* [M_out, Err] = SurfaceEquation(A_in, B_in, M_in, err_thr, min_set_size, iter [, seed])
 * Drop-in for mex/source/SurfaceEquation.c (reference gateway, -> RANSAC + mvarPolynomial): the RANSAC fit of a first- ([X Y 1])
 * or second-order ([X^2 Y^2 XY X Y 1]) polynomial surface A_in * M_out = B_in.  The six single arguments, the nlhs >= 2 rule and
 * the refusals are the reference's (:90-192), with its messages; an empty M_in means none.  Unlike the reference, which draws
 * rand() % ndata after one srand(time(NULL)), the samples come from a 64-bit seed (include/pdeip.h): the optional seventh argument
 * (a non-negative real scalar), or else a seed drawn from time() on the first call and advanced on every call. */
#include <time.h>

#include "../pdeip_mex_util.h"

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    static const char *who = "SurfaceEquation error";
    static unsigned long long next_seed;
    static int seeded = 0;
    const float *A, *B, *M;
    float err_thr, min_set_size, iter, *Mo, *Eo;
    unsigned long long seed;
    mwSize dims[2] = {0, 1};
    int ndata, ncoef;
    if (nrhs != 6 && nrhs != 7) mexErrMsgTxt("SurfaceEquation error: wrong number of input parameters!");
    A = pdeip_single(prhs[0], who, "A_in");
    B = pdeip_single(prhs[1], who, "B_in");
    M = pdeip_single(prhs[2], who, "M_in");
    err_thr = pdeip_scalar(prhs[3], who, "err_thr");
    min_set_size = pdeip_scalar(prhs[4], who, "min_set_size");
    iter = pdeip_scalar(prhs[5], who, "iter");
    if (nrhs == 7) {
        double v;
        if ((!mxIsDouble(prhs[6]) && !mxIsSingle(prhs[6])) || mxIsComplex(prhs[6]) || mxGetNumberOfElements(prhs[6]) != 1)
            mexErrMsgTxt("SurfaceEquation error: 'seed' must be a real scalar");
        v = mxIsDouble(prhs[6]) ? *(const double *)mxGetData(prhs[6]) : (double)*(const float *)mxGetData(prhs[6]);
        if (!(v >= 0.0 && v < 18446744073709551616.0)) mexErrMsgTxt("SurfaceEquation error: 'seed' must be in 0 .. 2^64 - 1");
        seed = (unsigned long long)v;
    } else {
        if (!seeded) {
            next_seed = (unsigned long long)time(NULL);
            seeded = 1;
        }
        seed = next_seed;
        next_seed += 0x9E3779B97F4A7C15ull;
    }
    if (mxGetNumberOfElements(prhs[2]) == 0) M = NULL;
    ndata = pdeip_rows(prhs[0]);
    ncoef = pdeip_cols(prhs[0]);
    if (M != NULL && ncoef != pdeip_rows(prhs[2]))
        mexErrMsgTxt("SurfaceEquation error: M_in is a column vector with as many row elements as A_in has columns!");
    if (ndata != pdeip_rows(prhs[1])) mexErrMsgTxt("SurfaceEquation error: A_in and B_in have to have same amount of rows!");
    if (ncoef != 3 && ncoef != 6) mexErrMsgTxt("SurfaceEquation error: only 1st and 2nd order polynomials are implemented!");
    if (nlhs < 2)
        mexErrMsgTxt("SurfaceEquation error: insufficient number of outputs. Outputs from this function is 'M_out' and 'error_out'");
    dims[0] = (mwSize)ncoef;
    plhs[0] = mxCreateNumericArray(2, dims, mxSINGLE_CLASS, mxREAL);
    Mo = (float *)mxGetData(plhs[0]);
    dims[0] = (mwSize)ndata;
    plhs[1] = mxCreateNumericArray(2, dims, mxSINGLE_CLASS, mxREAL);
    Eo = (float *)mxGetData(plhs[1]);
    /* (unsigned int)iter of the reference, without its wrap-around for a negative iter */
    pdeip_check(pdeip_surface_equation(A, B, ndata, ncoef, M, err_thr, min_set_size, iter > 0.0f ? (iter < 2147483648.0f ? (int)iter : 2147483647) : 0, NULL, seed, Mo, Eo, NULL,
                                       NULL));
}
