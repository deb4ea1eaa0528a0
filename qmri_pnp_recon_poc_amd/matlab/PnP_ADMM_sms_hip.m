function [x, lsqr_iters] = PnP_ADMM_sms_hip(y, maps, param)
% PNP_ADMM_SMS_HIP  PnP-ADMM of simultaneous multi-slice (SMS) groups on the GPU (extension, no reference counterpart): the loop of PnP_ADMM_hip
%   with the x-update solved over the Z slices of a group jointly, after qmri_set_sms(E).
%
%   y:    m x ncoil x G complex, one set of samples per group (the sum of its Z slices in every coil)
%   maps: N x M x ncoil x Z x G complex coil sensitivities, one set per slice
%   x:    N x M x s x Z x G;  lsqr_iters: iter x G (one LSQR count per group and ADMM iteration)
%   param: iter, gamma, cg_tol, denoiser_type, noise_map and net as PnP_ADMM_hip reads them (net from qmri_make_net, qmri_make_llr or
%   qmri_make_wavelet), tsmi_domain ('real' | 'complex'), X0 (N x M x s x Z x G; default: the adjoint of y) and groups_per_launch (default 1;
%   groups_per_launch * Z slice images go through the denoiser step at once).  Only the LSQR solver is built for coupled slices.
p.gamma = param.gamma;  p.iter = param.iter;  p.cg_tol = param.cg_tol;
llr = isstruct(param.net) && isfield(param.net, 'qmri_llr');
wav = isstruct(param.net) && isfield(param.net, 'qmri_wavelet');
p.multi_level = double(~llr && ~wav && isfield(param, 'denoiser_type') && strcmp(param.denoiser_type, 'multi_level'));
if p.multi_level, p.noise_std = param.noise_map(1); else, p.noise_std = 0.01; end
tsmi_domain = 'real';  if isfield(param, 'tsmi_domain'), tsmi_domain = char(param.tsmi_domain); end
if ~any(strcmp(tsmi_domain, {'real', 'complex'})), error('qmri:tsmi_domain', 'param.tsmi_domain must be ''real'' or ''complex'''); end
p.complex_tsmi = double(strcmp(tsmi_domain, 'complex'));
if isfield(param, 'solver') && ~(isequal(param.solver, 0) || strcmp(char(param.solver), 'lsqr'))
    error('qmri:solver', 'simultaneous multi-slice groups are solved by ''lsqr'' only');
end
groups_per_launch = 1;  if isfield(param, 'groups_per_launch'), groups_per_launch = double(param.groups_per_launch); end
X0 = [];  if isfield(param, 'X0') && ~isempty(param.X0), X0 = complex(double(param.X0)); end
[x, lsqr_iters] = qmri_mex('pnp_admm_sms', complex(double(maps)), complex(double(y)), p, X0, groups_per_launch);
end
