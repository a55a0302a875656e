/* pdeip_gac_mex.h -- the body both GAC driver stubs share: unpacking, checks, the pdeip_gac call. */
#ifndef PDEIP_GAC_MEX_H
#define PDEIP_GAC_MEX_H

#include <stdio.h>

static void pdeip_gac_mex(const char *who, int model, int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    char msg[256];
    const size_t np = model == PDEIP_GAC_A ? 5 : 4;
    pdeip_gac_params p;
    const float *I, *PHI;
    const double *pv;
    mwSize dims[2];
    int rows, cols;
    if (nrhs != 3) {
        snprintf(msg, sizeof msg, "%s parameter error: wrong number of input parameters!", who);
        mexErrMsgTxt(msg);
    }
    if (nlhs < 1) {
        snprintf(msg, sizeof msg, "%s insufficient number of outputs. Output from this function is 'PHIout'", who);
        mexErrMsgTxt(msg);
    }
    I = pdeip_single(prhs[0], who, "Iin");
    PHI = pdeip_single(prhs[1], who, "PHIin");
    rows = pdeip_rows(prhs[0]);
    cols = pdeip_cols(prhs[0]);
    if (mxGetNumberOfDimensions(prhs[1]) != 2 || pdeip_rows(prhs[1]) != rows || pdeip_cols(prhs[1]) != cols) {
        snprintf(msg, sizeof msg, "%s: 'PHIin' must be a [rows x cols] matrix of the image's size", who);
        mexErrMsgTxt(msg);
    }
    if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2]) || mxGetNumberOfElements(prhs[2]) != np) {
        snprintf(msg, sizeof msg, "%s: 'params' must be a real double vector of %d elements", who, (int)np);
        mexErrMsgTxt(msg);
    }
    pv = (const double *)mxGetData(prhs[2]);
    p.tau = pv[0];
    if (model == PDEIP_GAC_A) {
        p.c = pv[1];
        pv++;
    } else {
        p.c = 0.0; /* not a parameter of GAC_v10b */
    }
    p.lambda = pv[1];
    p.iter = pv[2];
    p.smooth = pv[3];
    dims[0] = (mwSize)rows;
    dims[1] = (mwSize)cols;
    plhs[0] = mxCreateNumericArray(2, dims, mxSINGLE_CLASS, mxREAL);
    pdeip_check(pdeip_gac(I, rows, cols, pdeip_frames(prhs[0]), PHI, model, &p, (float *)mxGetData(plhs[0])));
}

#endif
