/* Stand-in for MATLAB's mex.h: just enough of the MEX API for the reference's gateways to compile and run on a
 * host without MATLAB (oracle/build_ref.py).  Project-written; implemented in refmex.c.
 *
 * mwSize is 32 bits wide on purpose.  The reference's library reads array dimensions through 32-bit integer
 * pointers, as MATLAB's 32-bit array API (no -largeArrayDims) hands them out; a 64-bit mwSize would garble every
 * dimension after the first.  tests/test_ref_oracle.py checks the dimensions a gateway sees. */
#ifndef PDEIP_REFMEX_MEX_H
#define PDEIP_REFMEX_MEX_H

#include "matrix.h"

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]);
int mexPrintf(const char *fmt, ...);
void mexErrMsgTxt(const char *msg) __attribute__((noreturn)); /* returns to refmex_call() */

#endif
