function [It, Ut, Vt, src] = flow_interpolate_gpu(I0, I1, Uf, Vf, Ub, Vb, t, varargin)
%function [It, Ut, Vt, src] = flow_interpolate_gpu(I0, I1, Uf, Vf, Ub, Vb, t, varargin)
%
%The frame at time t (0 < t < 1) between the frames I0 and I1 from the flow (Uf, Vf) of frame 0 -> 1, on the GPU in one MEX call
%(mex/flow/flow_interpolate_gpu.c -> libpdeip.so pdeip_flow_interpolate): the baseline interpolation of Baker et al., IJCV 2011.
%The flow is carried forward to time t (where several pixels land on one, the most photo-consistent wins), the holes this leaves
%are filled by TV inpainting (TVinpaint4_gpu's parameters), and both frames are sampled along the flow at t and blended.  With the
%backward flow (Ub, Vb) of frame 1 -> 0 the forward-backward checks (a, b as in flow_crosscheck_gpu) decide at an occlusion which
%frame alone is shown; pass [] for both to do without.
%It has the size of I0; Ut, Vt are the filled flow at t; src is 0 neither frame, 1 frame 0 alone, 2 frame 1 alone, 3 both blended.
%  It = flow_interpolate_gpu(I0, I1, U, V, Ub, Vb, 0.5, 'outer_iter', 5)
%NOT RUN IN THIS REPOSITORY (no MATLAB in its build image); the MEX entry is tested through a mock MEX runtime.
param.a = 0.01;
param.b = 0.5;
param.use_costs = 1;
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
[It, Ut, Vt, src] = flow_interpolate_mex(I0, I1, Uf, Vf, Ub, Vb, double(t), ...
    double([param.a param.b param.use_costs param.alpha param.omega param.outer_iter param.inner_iter param.solver ...
            param.scl_factor param.min_size param.cover param.guide_scale param.keep]));
