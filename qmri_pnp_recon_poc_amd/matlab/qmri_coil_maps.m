function [maps, img, lam, info] = qmri_coil_maps(calib, opts)
% QMRI_COIL_MAPS  Coil sensitivity maps from calibration data on the GPU (extension, no reference counterpart).
%   The adaptive-combine estimator of Walsh, Gmitro & Marcellin (MRM 2000): per pixel the dominant eigenvector of the coil covariance summed over a
%   (2p + 1) x (2p + 1) patch of the calibration images.  The step between qmri_coil_compress and a multi-coil reconstruction.
%
%       F = qmri_make_F('Spiral', N, M, spiral_sampling_curve, V);        % the operator fixes N and M
%       maps = qmri_coil_maps(acs, struct('thresh', 0.05));               % acs: cN x cM x ncoil x S centred k-space block
%
%   calib: kind 'kspace' (default): cN x cM x ncoil x S complex, a centred block of k-space in the operator's convention (the centre crop of
%   fftshift(fft2(C_j x)) / sqrt(N M), index (cN/2 + 1, cM/2 + 1) is k = 0), cN and cM even, 8 <= cN <= N, 8 <= cM <= M; kind 'images':
%   N x M x ncoil x S calibration images.  ncoil <= 128.
%   opts (all optional): kind ('kspace' | 'images'), patch (half-width p, 0..4, default 3), window (Hann taper of the block, default true),
%   phase_ref ('object': maps' * I real and non-negative, the object's phase lives in the maps -- for real TSMIs; 'coil': the strongest coil real and
%   non-negative, the object's phase stays in x -- for param.tsmi_domain = 'complex'), thresh (pixels with lambda_1 < thresh^2 max lambda_1 are
%   zeroed; default 0 keeps all).
%   maps: N x M x ncoil x S, unit 2-norm over the coils on the pixels kept; img: N x M x S, the combined image; lam: N x M x S, lambda_1;
%   info: struct (max_iters, not_converged) of the per-pixel power iteration.
if nargin < 2, opts = struct(); end
o.images = 0; o.patch = 3; o.window = 1; o.phase_coil = 0; o.thresh = 0;
if isfield(opts, 'kind')
    switch lower(opts.kind)
        case 'kspace', o.images = 0;
        case 'images', o.images = 1;
        otherwise, error('qmri:coil_maps:opts', 'opts.kind must be ''kspace'' or ''images''');
    end
end
if isfield(opts, 'phase_ref')
    switch lower(opts.phase_ref)
        case 'object', o.phase_coil = 0;
        case 'coil', o.phase_coil = 1;
        otherwise, error('qmri:coil_maps:opts', 'opts.phase_ref must be ''object'' or ''coil''');
    end
end
if isfield(opts, 'patch'), o.patch = double(opts.patch); end
if isfield(opts, 'window'), o.window = double(logical(opts.window)); end
if isfield(opts, 'thresh'), o.thresh = double(opts.thresh); end
[maps, img, lam, info] = qmri_mex('coil_maps', complex(double(calib)), o);
end
