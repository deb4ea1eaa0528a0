function info = qmri_prepare_normal_fm(nseg, tol)
% QMRI_PREPARE_NORMAL_FM  Build the Toeplitz normal operator of a trajectory operator WITH a field map (extension, no reference counterpart).
%   With a map attached (qmri_set_field_map) every forward and adjoint is nseg NUFFTs, and the Toeplitz normal operator is refused until this call
%   has built its field-aware form: A'*A ~ sum_l P_l' * T_l * P_l from a segmentation of the difference phase exp(1i*2*pi*(f(n)-f(n'))*t)
%   (Fessler et al. 2005), each term the plain Toeplitz apply between two phase multiplies.
%
%       F = qmri_make_F_traj(N, M, V, frame_ptr, omega);
%       qmri_set_field_map(f, t);
%       info = qmri_prepare_normal_fm();                                   % as many segments as fit_max <= 1e-4 needs
%       z = qmri_mex('normal', x);   param.solver = 'toeplitz';            % now run with the map
%
%   nseg: segments, 2..32 (default 0: the smallest whose fit_max <= tol; expect about 2*L - 1 for the accuracy of an L-segment map);
%   tol: for nseg = 0 (default 0 = 1e-4).  info: struct (nseg, tol_reached, fit_max, fit_rms, khat_bytes: the transform's size on the device).
%   A constant map reports nseg = 1 and uses the plain transform.  A new map, clearing the map, or making a new operator drops the transform:
%   call again after them.  PnP_ADMM_hip does it before the loop when param.field_normal is set.
if nargin < 1 || isempty(nseg), nseg = 0; end
if nargin < 2 || isempty(tol), tol = 0; end
info = qmri_mex('prepare_normal_fm', double(nseg), double(tol));
end
