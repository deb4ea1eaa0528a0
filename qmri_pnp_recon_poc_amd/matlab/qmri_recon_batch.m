function [X, qmap, pd] = qmri_recon_batch(Y, param, devs, slices_per_launch)
% QMRI_RECON_BATCH  A whole slice stack through PnP-ADMM (+ the dictionary match) on the GPUs of one node.
%   The reference reconstructs one slice per run of main_recon_tsmis_FFT.m (:37-38, :293, :317); slices are independent, so a stack of S
%   slices is sharded over the devices in `devs` -- one worker (host thread + context) per entry, no communication between them -- and
%   on each device slices_per_launch slices advance together through the batched kernels:
%
%       F         = qmri_make_F('Spiral', N, M, spiral_sampling_curve, V);
%       param.net = qmri_make_net(denoiser_path, param.denoiser_type, residual_noise);
%       mrf_dtm_hip(dict, [], []);                        % (or any earlier call: leaves the dictionary set; optional)
%       [X, qmap, pd] = qmri_recon_batch(Y, param, 0:7, 15);     % Y: m x S, column j = F.forward(X0_j) + noise
%
%   X: N x M x s x S complex double (PnP_ADMM's x of every slice); qmap: N x M x Q x S single and pd: N x M x S complex single (mrf_dtm_cpu's
%   out.qmap / out.pd of every slice; empty when no dictionary is set or they are not asked for).
%   devs (default 0): device ids, an id may repeat (two workers sharing one GPU); slices_per_launch (default 15).
%   param: the reference's fields iter, gamma, cg_tol, denoiser_type, noise_map (PnP_ADMM.m:62-76); param.F from qmri_make_F.
%   param.tsmi_domain (optional): 'real' (default) or 'complex' -- complex TSMIs, the denoiser then takes 2s (+1) -> 2s channels.
%   param.coils (optional, multi-coil extension with no reference counterpart): N x M x ncoil x S coil maps, one set per slice; Y is then
%   m x ncoil x S, column (:, j, k) = F.forward(param.coils(:, :, j, k) .* X0_k) + noise.
%   param.coil_compress (optional, with param.coils): nv, or a struct with field nv -- every launch compresses its slices to nv virtual coils on
%   the GPU first, one transform per slice (qmri_coil_compress); param.noise_cov (optional): ncoil x ncoil noise covariance, whitened first.
if nargin < 3 || isempty(devs), devs = 0; end
if nargin < 4 || isempty(slices_per_launch), slices_per_launch = 15; end
if ~isfield(param.F, 'qmri'), error('qmri:F', 'param.F must be created by qmri_make_F'); end
p.gamma = param.gamma;  p.iter = param.iter;  p.cg_tol = param.cg_tol;
p.multi_level = double(strcmp(param.denoiser_type, 'multi_level'));
if p.multi_level, p.noise_std = param.noise_map(1); else, p.noise_std = 0.01; end
tsmi_domain = 'real';  if isfield(param, 'tsmi_domain'), tsmi_domain = char(param.tsmi_domain); end
if ~any(strcmp(tsmi_domain, {'real', 'complex'})), error('qmri:tsmi_domain', 'param.tsmi_domain must be ''real'' or ''complex'''); end
p.complex_tsmi = double(strcmp(tsmi_domain, 'complex'));   % complex TSMIs: the denoiser sees cat(3, real, imag), 2s (+1) -> 2s channels
g = param.F.qmri;
tail = {};
if isfield(param, 'coils') && ~isempty(param.coils)
    % multi-coil EXTENSION (no reference counterpart): param.coils N x M x ncoil x S (every slice its own maps), Y m x ncoil x S
    a = {'recon_batch_mc', complex(double(Y)), complex(double(param.coils))};
    if isfield(param, 'coil_compress') && ~isempty(param.coil_compress)
        cc = param.coil_compress;
        if ~isstruct(cc), cc = struct('nv', double(cc)); end
        psi = [];
        if isfield(param, 'noise_cov') && ~isempty(param.noise_cov), psi = complex(double(param.noise_cov)); end
        tail = {cc, psi};
    end
else
    a = {'recon_batch', complex(double(Y))};
end
if nargout > 1
    [X, qmap, pd] = qmri_mex(a{:}, p, double(devs(:)), double(slices_per_launch), [g.N g.M g.s], tail{:});
else
    X = qmri_mex(a{:}, p, double(devs(:)), double(slices_per_launch), [g.N g.M g.s], tail{:});
end
end
