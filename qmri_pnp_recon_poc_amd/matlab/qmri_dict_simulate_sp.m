function F = qmri_dict_simulate_sp(alpha, tr, te, t1, t2, prof, w, params, b1)
% QMRI_DICT_SIMULATE_SP  qmri_dict_simulate integrated over a slice profile on the GPU (extension, no reference counterpart).
%   A slice-selective pulse turns the magnetisation by a flip angle that varies through the slice; a voxel's signal is the integral over that
%   distribution.  The slice is cut into Q sub-slices (1 <= Q <= 64) with weights w and flip-angle scales prof:
%
%       F(k, t) = sum_q w(q) * (the fingerprint of atom k with the flip angles alpha(t) * b1(k) * prof(q, t))
%
%   summed on the GPU: no K x T x Q array is ever made.
%
%       F    = qmri_dict_simulate_sp(alpha, 0.012, 0.002, T1(:), T2(:), prof, ones(Q, 1) / Q, struct('nstates', 64));
%       dict = qmri_dict_compress(F, struct('s', 10), [T1(:) T2(:)]);
%
%   alpha, tr, te, t1, t2, params, b1: as in qmri_dict_simulate.  prof: Q x 1 (the same scale in every frame) or Q x T (one column per frame);
%   w: Q weights (default ones(Q, 1) / Q); every entry of both finite and >= 0, sum(w) > 0; the weights are not normalised.  F: K x T.
%   prof = 1, w = 1 gives qmri_dict_simulate's result bit for bit.
if nargin < 7 || isempty(w), w = ones(size(prof, 1), 1) / size(prof, 1); end
if nargin < 8 || isempty(params), params = struct(); end
if nargin < 9, b1 = []; end
if ~isreal(alpha) || ~isreal(t1) || ~isreal(t2) || ~isreal(b1)
    error('qmri:dict_simulate_sp:atoms', 'alpha, t1, t2 and b1 must be real');
end
if ~isreal(prof) || ~isreal(w)
    error('qmri:dict_simulate_sp:profile', 'prof and w must be real');
end
if isvector(prof), prof = prof(:); end
p = struct();
names = {'nstates', 'inversion', 'ti', 'inv_eff', 'single'};
for k = 1:numel(names)
    if isfield(params, names{k}), p.(names{k}) = double(params.(names{k})); end
end
F = qmri_mex('dict_simulate_sp', double(alpha(:)), double(tr(:)), double(te(:)), double(t1(:)), double(t2(:)), double(b1(:)), p, double(prof), double(w(:)));
end
