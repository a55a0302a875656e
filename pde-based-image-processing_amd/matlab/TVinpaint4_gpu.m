function [Dout, filled] = TVinpaint4_gpu(D, guide, varargin)
%function [Dout, filled] = TVinpaint4_gpu(D, guide, varargin)
%
%Fills the holes (NaN) of a sparse disparity or flow map on the GPU in one MEX call (mex/denoising/TVinpaint4_gpu.c -> libpdeip.so
%pdeip_tv_inpaint4): total-variation inpainting with PDEsolver4, whose NaN-TRACE branch fills a pixel by diffusion from its
%neighbours, and the lagged-diffusivity weights of TVdenoise4, coarse to fine over a NaN-aware pyramid.  D is [rows x cols] or
%[rows x cols x frames] (a flow: cat(3, U, V)), e.g. the sparse map of disp_crosscheck_gpu.  guide is an image on D's frame whose
%edges (times guide_scale) join the weights, so a filled region ends where the image says it does; [] for none.
%Dout has no NaN left; filled is 1 where D was a hole.  With keep = 1 the known pixels come back with their own bits.
%  TVinpaint4_gpu(D, I, 'alpha', 5, 'outer_iter', 10, 'guide_scale', 20)
%NOT RUN IN THIS REPOSITORY (no MATLAB in its build image); the MEX entry is tested through a mock MEX runtime.
param.alpha = 5;
param.omega = 1.75;
param.outer_iter = 10;
param.inner_iter = 5;
param.solver = 2;
param.scl_factor = 0.75;
param.min_size = 16;
param.cover = 0.25;
param.guide_scale = 20;
param.keep = 1;
param = setParameters(param, varargin{:});
[Dout, filled] = TVinpaint4_mex(D, guide, double([param.alpha param.omega param.outer_iter param.inner_iter param.solver ...
                                                   param.scl_factor param.min_size param.cover param.guide_scale param.keep]));
