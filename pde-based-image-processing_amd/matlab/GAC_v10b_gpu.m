function [PHIout] = GAC_v10b_gpu(Iin, PHIin, varargin)
%function [PHIout] = GAC_v10b_gpu(Iin, PHIin, varargin)
%
%Same call as GAC_v10b (matlab/active_contour/GAC_v10b.m of the toolbox); the whole run happens on the GPU in one MEX call
%(mex/levelset/GAC_v10b_gpu.c -> libpdeip.so pdeip_gac).  No figure is drawn.
%NOT RUN IN THIS REPOSITORY (no MATLAB in its build image); the MEX entry is tested through a mock MEX runtime.
param.tau = NaN; param.PHI = []; param.lambda = NaN; param.ITER = NaN; param.SMOOTH = NaN;	%NaN = the driver's default
param = setParameters(param, varargin{:});
PHIout = GAC_v10b_mex(single(Iin), single(PHIin), double([param.tau param.lambda param.ITER param.SMOOTH]));
