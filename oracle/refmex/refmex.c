/* Stand-in MEX runtime (see mex.h): arrays, zero-filled creation, mexErrMsgTxt as a longjmp back to refmex_call(),
 * and a small C entry set for tests/ref_lib.py (ctypes).  Linked into every oracle/_ref/<Gateway>.so. */
#include <setjmp.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mex.h"

#define REFMEX_MAX_DIMS 8

struct refmex_array {
    mwSize ndim;
    mwSize dims[REFMEX_MAX_DIMS];
    mxClassID classid;
    void *data;
};

static jmp_buf g_jmp;
static int g_armed;
static char g_err[1024];

static size_t elsize(mxClassID c) { return c == mxSINGLE_CLASS ? 4 : 8; }

static size_t numel(const mxArray *a)
{
    size_t n = 1;
    for (mwSize k = 0; k < a->ndim; k++) n *= a->dims[k];
    return n;
}

bool mxIsSingle(const mxArray *a) { return a->classid == mxSINGLE_CLASS; }
double *mxGetPr(const mxArray *a) { return (double *)a->data; }
const mwSize *mxGetDimensions(const mxArray *a) { return a->dims; }
mwSize mxGetNumberOfDimensions(const mxArray *a) { return a->ndim; }

/* As MATLAB does: at least two dimensions, and trailing singleton dimensions beyond the second dropped. */
mxArray *mxCreateNumericArray(mwSize ndim, const mwSize *dims, mxClassID classid, mxComplexity flag)
{
    (void)flag;
    if (ndim > REFMEX_MAX_DIMS) return NULL;
    mxArray *a = (mxArray *)calloc(1, sizeof *a);
    if (!a) return NULL;
    for (mwSize k = 0; k < REFMEX_MAX_DIMS; k++) a->dims[k] = k < ndim ? dims[k] : 1;
    a->ndim = ndim < 2 ? 2 : ndim;
    while (a->ndim > 2 && a->dims[a->ndim - 1] == 1) a->ndim--;
    a->classid = classid;
    a->data = calloc(numel(a) ? numel(a) : 1, elsize(classid));
    if (!a->data) {
        free(a);
        return NULL;
    }
    return a;
}

void *mxCalloc(size_t n, size_t size) { return calloc(n ? n : 1, size ? size : 1); }
void mxFree(void *p) { free(p); }

int mexPrintf(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    int n = vprintf(fmt, ap);
    va_end(ap);
    return n;
}

void mexErrMsgTxt(const char *msg)
{
    snprintf(g_err, sizeof g_err, "%s", msg);
    if (!g_armed) {
        fprintf(stderr, "refmex: mexErrMsgTxt outside refmex_call: %s\n", g_err);
        abort();
    }
    longjmp(g_jmp, 1);
}

/* ---- entry set for tests/ref_lib.py -------------------------------------------------------------------------- */

/* A new array of class `classid` (mxSINGLE_CLASS or mxDOUBLE_CLASS) with a copy of `data` (column-major). */
mxArray *refmex_make(int classid, int ndim, const long long *dims, const void *data)
{
    mwSize d[REFMEX_MAX_DIMS];
    if (ndim < 0 || ndim > REFMEX_MAX_DIMS) return NULL;
    for (int k = 0; k < ndim; k++) {
        if (dims[k] < 0 || dims[k] > 0xffffffffLL) return NULL;
        d[k] = (mwSize)dims[k];
    }
    mxArray *a = mxCreateNumericArray((mwSize)ndim, d, (mxClassID)classid, mxREAL);
    if (a && data) memcpy(a->data, data, numel(a) * elsize(a->classid));
    return a;
}

void refmex_free(mxArray *a)
{
    if (a) {
        free(a->data);
        free(a);
    }
}

int refmex_class(const mxArray *a) { return (int)a->classid; }
int refmex_ndim(const mxArray *a) { return (int)a->ndim; }
long long refmex_dim(const mxArray *a, int k) { return k >= 0 && k < (int)a->ndim ? (long long)a->dims[k] : 1; }
void *refmex_data(const mxArray *a) { return a->data; }
int refmex_mwsize_bytes(void) { return (int)sizeof(mwSize); }
const char *refmex_error(void) { return g_err; }

/* Call the gateway's mexFunction as MATLAB does.  0: returned; 1: it called mexErrMsgTxt (message in refmex_error()).
 * plhs must hold nlhs NULLs on entry; whatever the gateway created there before an error is the caller's to free. */
int refmex_call(int nlhs, mxArray **plhs, int nrhs, const mxArray **prhs)
{
    g_err[0] = 0;
    if (setjmp(g_jmp)) {
        g_armed = 0;
        return 1;
    }
    g_armed = 1;
    mexFunction(nlhs, plhs, nrhs, prhs);
    g_armed = 0;
    return 0;
}
