/* PHI_out = CV_solver_2d(PHI_in, D_in, DH_in, GradNorm_in, tau, nu)
 * Drop-in for mex/source/CV_solver_2d.c (reference gateway, -> CV_AOSOMP_4_2d): one AOS step of the Chan-Vese model.
 * Lines of any length are accepted (the reference refuses more than MAX_BUF_SIZE = 2048 rows or columns).  Unlike the
 * reference, which reads past the end of a smaller D_in, DH_in or GradNorm_in, the sizes are checked. */
#include "../pdeip_mex_util.h"

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    static const char *who = "cv_solver_2D error";
    const float *PHI, *D, *DH, *G;
    float tau, nu, *out;
    if (nrhs != 6) mexErrMsgTxt("cv_solver_2D parameter error: wrong number of input parameters!");
    PHI = pdeip_single(prhs[0], who, "PHI_in");
    D = pdeip_single(prhs[1], who, "D_in");
    DH = pdeip_single(prhs[2], who, "DH_in");
    G = pdeip_single(prhs[3], who, "GradNorm_in");
    tau = pdeip_scalar(prhs[4], who, "tau");
    nu = pdeip_scalar(prhs[5], who, "nu");
    if (mxGetNumberOfElements(prhs[1]) != mxGetNumberOfElements(prhs[0]) || mxGetNumberOfElements(prhs[2]) != mxGetNumberOfElements(prhs[0]) ||
        mxGetNumberOfElements(prhs[3]) != mxGetNumberOfElements(prhs[0]))
        mexErrMsgTxt("cv_solver_2D error: 'D_in', 'DH_in' and 'GradNorm_in' must have the size of 'PHI_in'.");
    if (nlhs < 1) mexErrMsgTxt("cv_solver_2D error insufficient number of outputs. Outputs from this function is 'PHI_out'");
    out = pdeip_out_like(&plhs[0], prhs[0]);
    pdeip_check(pdeip_cv_solver(PHI, D, DH, G, pdeip_rows(prhs[0]), pdeip_cols(prhs[0]), pdeip_frames(prhs[0]), tau, nu, out));
}
