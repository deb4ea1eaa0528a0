function [w, info] = qmri_dcf(niter, tol)
% QMRI_DCF  Density compensation weights of the trajectory operator on the GPU (extension, no reference counterpart).
%   The iteration of Pipe & Menon (MRM 1999) on the NUFFT's own interpolation kernel, all samples of all frames as one set, scaled so that
%   F.adjoint applied to w .* y has unit transfer where the trajectory has support (orthonormal V).  The weights are attached to the operator:
%
%       F = qmri_make_F_traj(N, M, V, frame_ptr, omega);                   % a trajectory operator
%       w = qmri_dcf();                                                    % 20 iterations
%       x = qmri_mex('adjoint_w', y);                                      % the gridding reconstruction A^H (w .* y), N x M x s
%       qmri_mex('set_sample_weights', w2);                                % ... or with the caller's own weights ([] clears them)
%
%   niter: iterations, 1..200 (default 0 = 20; wide kernels converge more slowly: at the default width 12 use 100 for a scale within 1 %).
%   tol: stop after the first iteration whose max |d - 1| is <= tol (default 0: never).
%   w: m x 1, the order of y; info: struct (iters, dev, clamped, split_tiles).
%   qmri_mex('adjoint', ...) and PnP_ADMM_hip ignore the weights; making a new operator drops them.
if nargin < 1 || isempty(niter), niter = 0; end
if nargin < 2 || isempty(tol), tol = 0; end
[w, info] = qmri_mex('dcf', double(niter), double(tol));
end
