function [x, diag, lsqr_iters, llr_tau] = PnP_ADMM_hip(y, param)
% PNP_ADMM_HIP  Drop-in for  x = PnP_ADMM(y, param)  (main_files/algorithms/PnP_ADMM/PnP_ADMM.m:1) that runs the whole
%   loop on the GPU (one boundary crossing per reconstruction).  param.F must come from qmri_make_F and param.net from
%   qmri_make_net; the fields read are the reference's own: iter, gamma, cg_tol, gt_tsmi, X0, denoiser_type, noise_map
%   (PnP_ADMM.m:62-76); param.net may instead be the struct of qmri_make_llr (the locally low-rank regulariser, DESIGN.md section 25: no network,
%   denoiser_type and noise_map are not read; the threshold used is the fourth output) or of qmri_make_wavelet (joint wavelet soft-thresholding,
%   DESIGN.md section 29: the same conventions, the same fourth output), and param.tsmi_domain ('real', the default and the reference's; 'complex': the denoiser sees
%   cat(3, real(x+u), imag(x+u)) and param.net must take 2s (+1) -> 2s channels), and param.solver ('lsqr', the default; 'direct'; 'toeplitz' on a
%   trajectory F: CG on the Toeplitz normal operator, DESIGN.md section 16), and param.field_normal (with a field map and solver 'toeplitz': true, or a
%   struct with nseg and / or tol, builds the field-aware normal operator before the loop, as qmri_prepare_normal_fm does).  Extra outputs: the two per-iteration diagnostics (PnP_ADMM.m:106-109) and the LSQR iteration counts.
%
%   y is the measurement vector of one slice (m x 1, as in the reference) or a measurement MATRIX m x S, one column per slice:
%   the S slices then advance together through the batched kernels (15 at a time) on the current device and x is
%   N x M x s x S (diag: S x iter x 2 -> returned as iter x 2 x S; lsqr_iters: iter x S); param.X0 / param.gt_tsmi, if given, are
%   N x M x s x S.  For S slices over SEVERAL GPUs see qmri_recon_batch.
if ~isfield(param.F, 'qmri'), error('qmri:F', 'param.F must be created by qmri_make_F'); end
p.gamma = param.gamma;  p.iter = param.iter;  p.cg_tol = param.cg_tol;
llr = isstruct(param.net) && isfield(param.net, 'qmri_llr');
wav = isstruct(param.net) && isfield(param.net, 'qmri_wavelet');
p.multi_level = double(~llr && ~wav && strcmp(param.denoiser_type, 'multi_level'));
if p.multi_level, p.noise_std = param.noise_map(1); else, p.noise_std = 0.01; end
tsmi_domain = 'real';  if isfield(param, 'tsmi_domain'), tsmi_domain = char(param.tsmi_domain); end
if ~any(strcmp(tsmi_domain, {'real', 'complex'})), error('qmri:tsmi_domain', 'param.tsmi_domain must be ''real'' or ''complex'''); end
p.complex_tsmi = double(strcmp(tsmi_domain, 'complex'));   % complex TSMIs: the denoiser sees cat(3, real, imag), 2s (+1) -> 2s channels
if isfield(param, 'solver')                                % 'lsqr' (default, the reference's), 'direct', 'toeplitz' (trajectory operators), or the integer
    sv = param.solver;
    if ischar(sv) || isstring(sv)
        k = find(strcmp(char(sv), {'lsqr', 'direct', 'toeplitz'}), 1);
        if isempty(k), error('qmri:solver', 'param.solver must be ''lsqr'', ''direct'', ''toeplitz'' or an integer'); end
        p.solver = k - 1;
    else
        p.solver = double(sv);
    end
end
if isfield(param, 'field_normal') && ~isempty(param.field_normal)  % true, or a struct with nseg / tol: qmri_prepare_normal_fm before the loop
    fn = param.field_normal;
    if isstruct(fn)
        if ~all(ismember(fieldnames(fn), {'nseg', 'tol'})), error('qmri:field_normal', 'param.field_normal must be true or a struct with nseg and / or tol'); end
        p.field_normal = 1;
        if isfield(fn, 'nseg'), p.field_normal_nseg = double(fn.nseg); end
        if isfield(fn, 'tol'), p.field_normal_tol = double(fn.tol); end
    elseif (islogical(fn) || isnumeric(fn)) && isscalar(fn)
        p.field_normal = double(fn ~= 0);
    else
        error('qmri:field_normal', 'param.field_normal must be true or a struct with nseg and / or tol');
    end
end
g = param.F.qmri;
if isvector(y), y = y(:); end
gt = [];  if isfield(param, 'gt_tsmi'), gt = complex(double(param.gt_tsmi)); end
X0 = [];  if isfield(param, 'X0'), X0 = complex(double(param.X0)); end
llr_tau = [];
if llr                                                     % Step 2 = the locally low-rank prox: threshold from the start image unless given
    llr_tau = param.net.tau;
    if isempty(llr_tau)
        start = X0;  if isempty(start), start = complex(double(param.F.adjoint(y(:, 1)))); end
        if ~p.complex_tsmi, start = real(start); end
        [~, smax] = qmri_mex('llr_prox', start, 0, param.net.block);
        llr_tau = param.net.tau_rel * max(smax);
    end
    qmri_mex('set_llr', llr_tau, param.net.block, param.net.shift);
    unset = onCleanup(@() qmri_mex('clear_llr'));
end
if wav                                                     % Step 2 = joint wavelet soft-thresholding: threshold from the start image unless given
    w = param.net;
    llr_tau = w.tau;
    if isempty(llr_tau)
        start = X0;  if isempty(start), start = complex(double(param.F.adjoint(y(:, 1)))); end
        if ~p.complex_tsmi, start = real(start); end
        [~, cmax] = qmri_mex('wavelet_prox', start, 0, w.levels, w.filter, w.joint);
        llr_tau = w.tau_rel * max(cmax);
    end
    qmri_mex('set_wavelet', llr_tau, w.levels, w.filter, w.joint, w.shift);
    unset = onCleanup(@() qmri_mex('clear_wavelet'));
end
if nargout > 1
    [x, diag, lsqr_iters] = qmri_mex('pnp_admm', complex(double(y)), p, X0, gt, [g.N g.M g.s]);
    diag = permute(diag, [2 1 3]);
else
    x = qmri_mex('pnp_admm', complex(double(y)), p, X0, gt, [g.N g.M g.s]);
end
end
