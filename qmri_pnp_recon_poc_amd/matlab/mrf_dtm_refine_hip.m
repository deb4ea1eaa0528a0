function out = mrf_dtm_refine_hip(dict, data, par, cols)
% MRF_DTM_REFINE_HIP  Dictionary match, then T1 / T2 moved off the dictionary's grid by a fit through neighbouring atoms.
%   An extension (no reference counterpart; include/qmri.h qmri_set_refine / qmri_dict_refine): mrf_dtm_cpu.m returns lut(dm, :), maps quantised to
%   the grid.  Every pixel is fitted to the quadratic through its matched atom and that atom's neighbours along each refined lut column.
%   dict, data, par  as for mrf_dtm_hip (dict.D K x s with s <= 16)
%   cols             the lut columns to refine, 1-based (default [1 2]: T1, T2), 1 to 3 of them
%   out              what mrf_dtm_hip returns (out.qmap, out.pd, ...: unchanged) and
%   out.qmap_refined [..., Q] double: refined columns off the grid, the others the lut value of the final centre atom
%   out.pd_refined   [...] complex double (x ~ pd * unnormalised atom, the match's convention)
%   out.refine_res   [...] = ||x - pd d|| / ||x||;  out.refine_t [..., P] the position between the neighbours, in [-1, 1]
%   out.refine_centre [...] int32, the 1-based atom the result is expressed around
%   out.refine_flags [...] int32: 1 skipped, 2 re-centred, 4 on a bound of its box, 8 iteration cap, 16 stalled, 32 degenerate (grid values)
%   out.refine_info  P, K, s, count (P x 3: atoms with 0, 1, 2 neighbours along each refined column)
if nargin < 4 || isempty(cols), cols = [1 2]; end
if numel(cols) < 1 || numel(cols) > 3 || any(cols(:) ~= floor(cols(:))) || any(cols(:) < 1) || any(cols(:) > size(dict.lut, 2))
    error('qmri:refine:cols', 'cols must be 1 to 3 columns of dict.lut (1-based)');
end
datadims = size(data.X); T = datadims(end); Npix = prod(datadims(1:end-1)); lead = datadims(1:end-1);
Q = size(dict.lut, 2);
out = mrf_dtm_hip(dict, data, par);      % leaves the dictionary set
X = complex(double(reshape(data.X, [Npix, T])));
if isfield(out, 'dm')
    dm = int32(out.dm(:));
else
    [~, ~, ~, dm] = qmri_mex('dict_match', X, Q);
end
out.refine_info = qmri_mex('set_refine', double(cols(:)) - 1);
[qmap, pd, res, t, centre, flags] = qmri_mex('dict_refine', X, int32(dm(:)));
out.qmap_refined = reshape(qmap, [lead, Q]);
out.pd_refined = reshape(pd, [lead, 1]); out.refine_res = reshape(res, [lead, 1]);
out.refine_t = reshape(t, [lead, numel(cols)]);
out.refine_centre = reshape(centre, [lead, 1]); out.refine_flags = reshape(flags, [lead, 1]);
end
