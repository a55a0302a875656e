function [mask, err, stats] = flow_crosscheck_gpu(flowF, flowB, varargin)
%function [mask, err, stats] = flow_crosscheck_gpu(flowF, flowB, varargin)
%
%Forward-backward check of two flows on the GPU in one MEX call (mex/flow/flow_crosscheck_gpu.c -> libpdeip.so
%pdeip_flow_crosscheck).  flowF = cat(3, U, V) of frame 0 -> 1, flowB that of frame 1 -> 0 (the same driver with the frames swapped).
%A pixel is kept when |f + b(x+f)|^2 <= a (|f|^2 + |b(x+f)|^2) + b, the criterion of Sundaram, Brox and Keutzer (ECCV 2010) with
%their a = 0.01, b = 0.5 as defaults: flow_crosscheck_gpu(F, B, 'a', 0, 'b', 1) is an absolute threshold of one pixel.
%mask is 1 / 0, err is |f + b(x+f)| (NaN where x + f leaves the picture), stats = [kept defined mean max] of err.
%NOT RUN IN THIS REPOSITORY (no MATLAB in its build image); the MEX entry is tested through a mock MEX runtime.
param.a = 0.01;
param.b = 0.5;
param = setParameters(param, varargin{:});
[mask, err, stats] = flow_crosscheck_mex(flowF, flowB, double([param.a param.b]));
