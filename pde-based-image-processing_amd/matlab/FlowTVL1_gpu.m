function [U, V] = FlowTVL1_gpu(Iin, varargin)
%function [U, V] = FlowTVL1_gpu(Iin, varargin)
%
%TV-L1 optical flow on the GPU (Zach, Pock and Bischof; the first-order primal-dual iteration of Chambolle and Pock), warped and
%coarse to fine, in one MEX call (mex/flow/FlowTVL1_gpu.c -> libpdeip.so pdeip_flow_tvl1).  Iin = cat(3, frame0, frame1), gray, 0..255.
%  lambda      the data weight (default 15)
%  warps       linearisations per scale (default 3)
%  iter        primal-dual iterations per warp (default 20)
%  huber       0 (default) = TV; > 0 = the Huber norm
%  scl_factor  the pyramid's factor (default 0.75); scales: the number of scales (default: down to a side of 20 pixels)
%  tau, sigma  the step sizes (defaults 0.25 and 0.5; tau * sigma * 8 must not exceed 1)
%  [U, V] = FlowTVL1_gpu(cat(3, I0, I1), 'lambda', 15, 'warps', 3, 'iter', 20)
%A colour pair: hand over its gray pair, e.g. cat(3, mean(single(A), 3), mean(single(B), 3)).
%NOT RUN IN THIS REPOSITORY (no MATLAB in its build image); the MEX entry is tested through a mock MEX runtime.
param.lambda = 15;
param.warps = 3;
param.iter = 20;
param.huber = 0;
param.scl_factor = 0.75;
param.scales = 0;
param.tau = NaN;
param.sigma = NaN;
param = setParameters(param, varargin{:});
[U, V] = FlowTVL1_mex(Iin, double([param.lambda param.huber param.tau param.sigma param.scl_factor param.warps param.iter param.scales]));
