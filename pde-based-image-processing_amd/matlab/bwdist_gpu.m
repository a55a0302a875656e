function [D, IDX] = bwdist_gpu(BW)
%function [D, IDX] = bwdist_gpu(BW)
%
%[D, IDX] = bwdist(BW) with the Euclidean metric on the GPU in one MEX call (mex/morph/bwdist_gpu.c -> libpdeip.so pdeip_bwdist).
%BW is a logical mask, or numbers of which the positive ones are the features.  D is the single distance to the nearest feature,
%IDX the uint32 1-based linear index of that feature (0 in a plane without one).  Among equidistant features the lowest index wins;
%whether MATLAB's own bwdist breaks every tie the same way is not pinned.
%NOT RUN IN THIS REPOSITORY (no MATLAB in its build image); the MEX entry is tested through a mock MEX runtime.
if nargout > 1
    [D, IDX] = bwdist_mex(single(BW > 0));
else
    D = bwdist_mex(single(BW > 0));
end
