function dict = qmri_dict_compress(F, params, lut)
% QMRI_DICT_COMPRESS  A simulated MRF dictionary compressed to its SVD subspace on the GPU (extension, no reference counterpart).
%   The reference loads dictionaries that are already compressed (SVD_dict_FISP_cut*.mat).  This takes what a Bloch / EPG simulator writes and
%   returns the fields those files hold:
%
%       dict = qmri_dict_compress(F, struct('s', 10), lut);               % F: K x T fingerprints, lut: K x 2 (T1, T2)
%       F_op = qmri_make_F('Spiral', N, M, spiral_sampling_curve, dict.V);
%       out  = mrf_dtm_hip(dict, data, par);
%
%   F: K x T real double or single, K fingerprints of T <= 1024 frames (single stays single on its way to the device).
%   params: struct with s (the rank, 1..16; the operator takes s <= 10) or energy (the fraction of trace(F' * F) to keep, in (0, 1], with at most
%   s_max <= 16 vectors, default 16); optional tol (residual bound of the eigenpairs relative to lambda_1, default 1e-13) and maxit (default 200).
%   lut (optional): copied into dict.lut.
%   dict: V (T x s double, orthonormal, each column's largest entry positive), D (K x s single, unit rows), normD (K x 1 single), eig (s x 1, the
%   leading eigenvalues of F' * F), info (s, iters, converged, energy_reached, max_resid, energy_kept), and lut when given.
if ~isreal(F), error('qmri:dict_compress:F', 'F must be real (complex fingerprints are not supported)'); end
if ~isa(F, 'single'), F = double(F); end
p = struct();
names = {'s', 's_max', 'energy', 'tol', 'maxit'};
for k = 1:numel(names)
    if isfield(params, names{k}), p.(names{k}) = double(params.(names{k})); end
end
[dict.V, dict.D, dict.normD, dict.eig, dict.info] = qmri_mex('dict_compress', F, p);
if nargin > 2, dict.lut = single(lut); end
end
