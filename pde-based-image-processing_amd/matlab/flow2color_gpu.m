function [img, maxvalue] = flow2color_gpu(flow, varargin)
%function [img, maxvalue] = flow2color_gpu(flow, varargin)
%
%Same call as flow2color (matlab/optical_flow/flow2color.m of the toolbox): I = flow2color_gpu(cat(3,U,V), 'border', 10); the colour
%coding happens on the GPU in one MEX call (mex/flow/flow2color_gpu.c -> libpdeip.so pdeip_flow2color).  img is single; maxvalue is
%the maximum magnitude used, which flow2color displays.  The picture is pasted into the frame at index param.border, as there.
%NOT RUN IN THIS REPOSITORY (no MATLAB in its build image); the MEX entry is tested through a mock MEX runtime.
param.maxvalue = [];
param.border = 0;
param = setParameters(param, varargin{:});
if isempty(param.maxvalue), param.maxvalue = NaN; end	%NaN = the function's default: max(mag(:))
[img, maxvalue] = flow2color_mex(flow, double([param.maxvalue param.border]));
