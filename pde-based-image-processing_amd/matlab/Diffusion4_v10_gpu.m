function [Iout] = Diffusion4_v10_gpu(I_in, varargin)
%function [Iout] = Diffusion4_v10_gpu(I_in, varargin)
%
%Same call as Diffusion4_v10 (matlab/diffusion/Diffusion4_v10.m of the toolbox); the whole run happens on the GPU in one MEX call
%(mex/diffusion/Diffusion4_v10_gpu.c -> libpdeip.so pdeip_diffusion4), and the result is cast to uint8 here, as the driver does.
%NOT RUN IN THIS REPOSITORY (no MATLAB in its build image); the MEX entry is tested through a mock MEX runtime.
param.alpha = NaN; param.outer_iter = NaN;	%NaN = the driver's default (25, 5)
param = setParameters(param, varargin{:});
Iout = uint8(Diffusion4_v10_mex(single(I_in), double([param.alpha param.outer_iter])));
