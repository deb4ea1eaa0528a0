function info = qmri_set_field_map(f, t, nseg, nbins, tol)
% QMRI_SET_FIELD_MAP  Attach a field map to the trajectory operator: off-resonance correction on the GPU (extension, no reference counterpart).
%   A pixel f Hz off resonance accumulates the phase 2*pi*f*t over a readout; for spirals this blurs the image.  With a map attached the operator
%   carries exp(-1i*2*pi*f(n)*t(i)), computed by time segmentation (Sutton, Noll & Fessler 2003) as nseg NUFFTs:
%
%       F = qmri_make_F_traj(N, M, V, frame_ptr, omega);                   % a trajectory operator
%       t = repmat((0:S-1)' * (readout_s / S), T, 1);                      % readout time of every sample, seconds, the order of y
%       info = qmri_set_field_map(f, t);                                   % f: N x M, Hz; as many segments as fit_max <= 1e-4 needs
%       x = PnP_ADMM_hip(...);                                             % forward, adjoint, the LSQR and PnP-ADMM all use the corrected operator
%       qmri_set_field_map([]);                                            % clears the map
%
%   nseg: segments, 1..16 (default 0: the smallest whose fit_max <= tol); nbins: histogram bins of the fit, 16..1024 (default 0 = 256);
%   tol: for nseg = 0 (default 0 = 1e-4).  info: struct (nseg, tol_reached, fit_max, fit_rms, f_min, f_max, t_min, t_max).
%   The cost is about nseg times the plain transform.  One map per operator (every coil and slice).  While a map is attached the Toeplitz normal
%   operator ('normal', solver 'toeplitz') is refused until qmri_prepare_normal_fm (or param.field_normal in PnP_ADMM_hip) has built its
%   field-aware form for this map; the LSQR needs no such call.  Making a new operator drops the map, as it drops the sample weights.
if isempty(f), qmri_mex('set_field_map', []); info = []; return; end
if nargin < 3 || isempty(nseg), nseg = 0; end
if nargin < 4 || isempty(nbins), nbins = 0; end
if nargin < 5 || isempty(tol), tol = 0; end
info = qmri_mex('set_field_map', double(f), double(t(:)), double(nseg), double(nbins), double(tol));
end
