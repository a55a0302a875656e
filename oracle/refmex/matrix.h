/* Stand-in for MATLAB's matrix.h (the mxArray half of the MEX API); see mex.h beside it. */
#ifndef PDEIP_REFMEX_MATRIX_H
#define PDEIP_REFMEX_MATRIX_H

#include <stdbool.h>
#include <stddef.h>

typedef unsigned int mwSize; /* 32-bit: see mex.h */
typedef struct refmex_array mxArray;
typedef enum { mxDOUBLE_CLASS = 6, mxSINGLE_CLASS = 7 } mxClassID;
typedef enum { mxREAL = 0, mxCOMPLEX = 1 } mxComplexity;

bool mxIsSingle(const mxArray *a);
double *mxGetPr(const mxArray *a); /* the data, whatever the class (callers cast) */
const mwSize *mxGetDimensions(const mxArray *a);
mwSize mxGetNumberOfDimensions(const mxArray *a);
mxArray *mxCreateNumericArray(mwSize ndim, const mwSize *dims, mxClassID classid, mxComplexity flag); /* zero-filled */
void *mxCalloc(size_t n, size_t size);
void mxFree(void *p);

#endif
