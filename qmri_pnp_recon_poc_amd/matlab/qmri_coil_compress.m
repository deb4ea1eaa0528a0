function [yc, mapsc, W, eig] = qmri_coil_compress(Y, maps, opts)
% QMRI_COIL_COMPRESS  Compress a multi-coil stack to nv virtual coils on the GPU (extension, no reference counterpart).
%   One linear map on the coil index, applied alike to the data and to the coil maps (Buehrer et al. 2007; Huang et al. 2008), optionally after
%   pre-whitening with a measured noise covariance.  The SENSE model is linear in the coil index, so the compressed stack reconstructs with the
%   same calls (qmri_recon_batch with param.coils = mapsc) at about nv / ncoil of the cost per x-update.
%
%       F = qmri_make_F('Spiral', N, M, spiral_sampling_curve, V);        % the operator fixes m, N and M
%       [yc, mapsc] = qmri_coil_compress(Y, maps, struct('nv', 8));
%
%   Y: m x ncoil x S complex (column (:, j, k) = coil j of slice k); maps: N x M x ncoil x S or [] (then mapsc = []).
%   opts (all optional): nv (> 0: keep nv virtual coils; 0 or absent: the smallest nv holding opts.energy of the eigenvalue sum, the largest over
%   the slices), energy (default 0.99), shared (true: one W for the whole stack; default: one per slice), noise_cov (ncoil x ncoil Hermitian
%   positive definite: whiten first).
%   yc: m x nv x S; mapsc: N x M x nv x S; W: ncoil x nv x S (x 1 when shared), yc(:, :, k) = Y(:, :, k) * conj(W(:, :, k)); eig: ncoil x S
%   (x 1 when shared), the eigenvalues of the (whitened) coil covariance, descending.  ncoil <= 128.
if nargin < 2, maps = []; end
if nargin < 3, opts = struct(); end
cc.nv = 0; cc.energy = 0.99; cc.shared = 0;
if isfield(opts, 'nv'), cc.nv = double(opts.nv); end
if isfield(opts, 'energy'), cc.energy = double(opts.energy); end
if isfield(opts, 'shared'), cc.shared = double(logical(opts.shared)); end
psi = [];
if isfield(opts, 'noise_cov') && ~isempty(opts.noise_cov), psi = complex(double(opts.noise_cov)); end
if ~isempty(maps), maps = complex(double(maps)); end
[yc, mapsc, W, eig] = qmri_mex('coil_compress', complex(double(Y)), maps, psi, cc);
end
