function [PHIout] = GAC_v10a_gpu(Iin, PHIin, varargin)
%function [PHIout] = GAC_v10a_gpu(Iin, PHIin, varargin)
%
%Same call as GAC_v10a (matlab/active_contour/GAC_v10a.m of the toolbox); the whole run happens on the GPU in one MEX call
%(mex/levelset/GAC_v10a_gpu.c -> libpdeip.so pdeip_gac).  No figure is drawn.
%NOT RUN IN THIS REPOSITORY (no MATLAB in its build image); the MEX entry is tested through a mock MEX runtime.
param.tau = NaN; param.PHI = []; param.c = NaN; param.lambda = NaN; param.ITER = NaN; param.SMOOTH = NaN;	%NaN = the driver's default
param = setParameters(param, varargin{:});
PHIout = GAC_v10a_mex(single(Iin), single(PHIin), double([param.tau param.c param.lambda param.ITER param.SMOOTH]));
