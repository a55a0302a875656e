function [Ds, mask, stats] = disp_crosscheck_gpu(D0, D1, tol)
%function [Ds, mask, stats] = disp_crosscheck_gpu(D0, D1, tol)
%
%Left-right check of two disparity maps on the GPU in one MEX call (mex/flow/disp_crosscheck_gpu.c -> libpdeip.so
%pdeip_disp_crosscheck).  D0 is the view being checked, D1 the other view, in the sign convention of DispEminND_llin_sym_2D: with
%U = DispEminND_llin_sym_2D(Il, Ir), Ds = disp_crosscheck_gpu(U(:,:,1), U(:,:,2)).  A pixel is kept when D1, sampled linearly at
%x + D0, cancels D0 to within tol pixels (default 1).  Ds is D0 with NaN where the pixel is not kept, as DispSegmentationSparse takes
%it; mask is 1 / 0; stats = [kept defined mean max] of |D0 + D1(x + D0)|.
%NOT RUN IN THIS REPOSITORY (no MATLAB in its build image); the MEX entry is tested through a mock MEX runtime.
if nargin < 3 || isempty(tol), tol = 1; end
[Ds, mask, stats] = disp_crosscheck_mex(D0, D1, double(tol));
