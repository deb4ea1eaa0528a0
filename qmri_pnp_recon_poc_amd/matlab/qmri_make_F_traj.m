function F = qmri_make_F_traj(N, M, V, frame_ptr, omega, width)
% QMRI_MAKE_F_TRAJ  GPU forward/adjoint operator on a non-Cartesian trajectory (a NUFFT; DESIGN.md section 14), with the plugin surface of
%   qmri_make_F:  F.forward(x) gives one sample per row of omega, F.adjoint(y) the N x M x s image, and PnP_ADMM_hip(y, param) with
%   param.F = F reconstructs from them (one slice at a time; no per-iteration diagnostics: that output is NaN).
%   omega      m x 2 radians per pixel in [-pi, pi]: column 1 along N (rows), column 2 along M; frame-major, frame f holding rows
%              frame_ptr(f)+1 : frame_ptr(f+1).  A trajectory k in cycles per field of view is omega = 2*pi*k.
%   frame_ptr  (T+1) x 1 int32, T = size(V, 1);  width (optional) the NUFFT kernel width, 0 or absent = the default.
if nargin < 6, width = 0; end
s = size(V, 2);
qmri_mex('set_trajectory', N, M, real(double(V)), int32(frame_ptr), double(omega), 1, width);
F.forward = @(x) qmri_mex('forward', double(x));
F.adjoint = @(y) qmri_mex('adjoint', complex(double(y)), [N M s]);
F.qmri = struct('N', N, 'M', M, 's', s);      % marks F as GPU resident for PnP_ADMM_hip
end
