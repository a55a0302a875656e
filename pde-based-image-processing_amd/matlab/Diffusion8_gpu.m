function [Iout] = Diffusion8_gpu(I_in, mode, varargin)
%function [Iout] = Diffusion8_gpu(I_in, mode, varargin)
%
%Structure-tensor anisotropic diffusion of I_in (0..255, gray or colour) in the call shape of Diffusion4_v10: mode 'ced'
%(coherence-enhancing, the default) or 'eed' (edge-enhancing), then name-value parameters sigma, rho, lambda, alpha, C, tau,
%iters, inner_iter, omega, solver.  The whole run happens on the GPU in one MEX call (mex/diffusion/Diffusion8_gpu.c ->
%libpdeip.so pdeip_diffusion8), and the result is cast to uint8 here, as Diffusion4_v10 does.
%NOT RUN IN THIS REPOSITORY (no MATLAB in its build image); the MEX entry is tested through a mock MEX runtime.
if nargin < 2 || isempty(mode), mode = 'ced'; end
param.sigma = NaN; param.rho = NaN; param.lambda = NaN; param.alpha = NaN; param.C = NaN; param.tau = NaN;	%NaN = the default of the mode
param.iters = NaN; param.inner_iter = NaN; param.omega = NaN; param.solver = NaN;
param = setParameters(param, varargin{:});
m = find(strcmpi(mode, {'eed', 'ced'})) - 1;
if isempty(m), error('Diffusion8_gpu: mode must be ''eed'' or ''ced'''); end
Iout = uint8(Diffusion8_mex(single(I_in), double([m param.sigma param.rho param.lambda param.alpha param.C param.tau ...
                            param.iters param.inner_iter param.omega param.solver])));
