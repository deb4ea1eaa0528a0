function [b1, out] = qmri_b1_estimate(dict, X, mask, half_window)
% QMRI_B1_ESTIMATE  The B1 map of a TSMI estimated from the fingerprints themselves, for protocols without a separate B1 scan.
%   An extension (no reference counterpart; include/qmri.h qmri_b1_estimate).  Per pixel the b1 group of the dictionary whose best atoms explain
%   the most energy over a (2*half_window+1)^2 window; T1, T2 and PD stay free per pixel.
%   dict as for mrf_dtm_b1_hip (dict.group_ptr, dict.group_val);  X  N x M x s or N x M x nslices x s;  mask ([]: every pixel) non-zero = foreground;
%   half_window (default 4) in 0 .. 32.
%   b1  N x M (x nslices), NaN where nothing was estimated -- what mrf_dtm_b1_hip takes as data.B1 (NaN: background).
%   out.grp (1-based group, 0 none), out.conf ((P_best - P_second) / P_best), out.info (n_estimated, n_unmatched, mean_conf).
if nargin < 3, mask = []; end
if nargin < 4, half_window = 4; end
dims = size(X); T = dims(end); lead = dims(1:end-1);
if numel(lead) < 2 || numel(lead) > 3
    error('qmri:b1_estimate:size', 'X must be N x M x s or N x M x nslices x s');
end
Npix = prod(lead);
if ~isempty(mask) && numel(mask) ~= Npix
    error('qmri:b1_estimate:size', 'mask must hold one value per pixel of X');
end
mrf_dtm_hip(dict, [], []);      % leaves the dictionary set (and checks dict.D)
qmri_mex('set_dictionary_groups', double(dict.group_ptr(:)), double(dict.group_val(:)));
shape = [lead(1), lead(2), prod(lead(3:end))];
[b1, grp, conf, info] = qmri_mex('b1_estimate', complex(double(reshape(X, [Npix, T]))), double(shape), double(mask(:) ~= 0), double(half_window));
b1 = reshape(b1, [lead, 1]);
out.grp = reshape(grp, [lead, 1]);
out.conf = reshape(conf, [lead, 1]);
out.info = info;
end
