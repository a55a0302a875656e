/* PHI_out = AC_solver_2d(PHI_in, D_in, GradNorm_in, Diff_in, tau, nu)
 * Drop-in for mex/source/AC_solver_2d.c (reference gateway :47-228): one AOS step of the geodesic active contour.
 * Lines of any length are accepted (the reference refuses more than MAX_BUF_SIZE = 2048 rows or columns). */
#include "../pdeip_mex_util.h"

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    static const char *who = "AC_solver_2D error";
    const float *PHI, *D, *G, *Df;
    float tau, nu, *out;
    if (nrhs != 6) mexErrMsgTxt("AC_solver_2D parameter error: wrong number of input parameters!");
    PHI = pdeip_single(prhs[0], who, "PHI_in");
    D = pdeip_single(prhs[1], who, "D_in");
    G = pdeip_single(prhs[2], who, "GradNorm_in");
    Df = pdeip_single(prhs[3], who, "Diff_in");
    tau = pdeip_scalar(prhs[4], who, "tau");
    nu = pdeip_scalar(prhs[5], who, "nu");
    if (mxGetNumberOfElements(prhs[1]) != mxGetNumberOfElements(prhs[0]) || mxGetNumberOfElements(prhs[2]) != mxGetNumberOfElements(prhs[0]) ||
        mxGetNumberOfElements(prhs[3]) != mxGetNumberOfElements(prhs[0]))
        mexErrMsgTxt("AC_solver_2D error: 'D_in', 'GradNorm_in' and 'Diff_in' must have the size of 'PHI_in'.");
    if (nlhs < 1) mexErrMsgTxt("ac_solver_2D error insufficient number of outputs. Outputs from this function is 'PHI_out'");
    out = pdeip_out_like(&plhs[0], prhs[0]);
    pdeip_check(pdeip_ac_solver(PHI, D, G, Df, pdeip_rows(prhs[0]), pdeip_cols(prhs[0]), pdeip_frames(prhs[0]), tau, nu, out));
}
