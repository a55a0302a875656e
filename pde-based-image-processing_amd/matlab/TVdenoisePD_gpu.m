function Iout = TVdenoisePD_gpu(I, varargin)
%function Iout = TVdenoisePD_gpu(I, varargin)
%
%Total-variation denoising on the GPU by the first-order primal-dual iteration of Chambolle and Pock, in one MEX call
%(mex/denoising/TVdenoisePD_gpu.c -> libpdeip.so pdeip_tv_pd).  I is [rows x cols] or [rows x cols x frames]; NaN means no data.
%  model    'l1' (default): TV + lambda |u - I|, which rejects gross outliers; 'l2': TV + lambda/2 (u - I)^2 (ROF)
%  lambda   the data weight (default 0.8)
%  huber    0 (default) = TV; > 0 = the Huber norm, which takes the staircase out of slopes
%  iter     iterations (default 300)
%  u0       the start ([] = I with its holes filled from the nearest known pixel)
%  tau, sigma   the step sizes (NaN = 0.25 and 0.5; tau * sigma * 8 must not exceed 1)
%  TVdenoisePD_gpu(D, 'model', 'l1', 'lambda', 0.8, 'iter', 300)
%NOT RUN IN THIS REPOSITORY (no MATLAB in its build image); the MEX entry is tested through a mock MEX runtime.
param.model = 'l1';
param.lambda = 0.8;
param.huber = 0;
param.iter = 300;
param.u0 = [];
param.tau = NaN;
param.sigma = NaN;
param = setParameters(param, varargin{:});
model = find(strcmpi(param.model, {'l1', 'l2'})) - 1;
if isempty(model)
    error('TVdenoisePD_gpu: model must be ''l1'' or ''l2''');
end
Iout = TVdenoisePD_mex(I, param.u0, double([model param.lambda param.huber param.iter param.tau param.sigma]));
