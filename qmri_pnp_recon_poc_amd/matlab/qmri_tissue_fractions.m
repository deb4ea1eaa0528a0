function out = qmri_tissue_fractions(dict, X, components, mode)
% QMRI_TISSUE_FRACTIONS  Tissue-fraction (partial-volume) maps: every pixel as a non-negative mix of a few chosen dictionary atoms.
%   An extension (the reference's mrf_dtm_cpu.m gives every pixel one atom; partial-volume MRF: Deshmane et al. 2019).
%   dict        as for mrf_dtm_hip (dict.D K x s with s <= 16, dict.normD, dict.lut with T1, T2 in its first two columns)
%   X           the TSMI, [..., s], real or complex
%   components  C x 2 (T1, T2) pairs in the units of dict.lut (each stands for the nearest atom, the first minimum winning), or a COLUMN vector
%               of 1 <= C <= 8 atom indices (1-based)
%   mode        'real' (default): the real part of X is fitted;  'phase': the pixel's own phase is removed first
%   out.frac [..., C] = w ./ sum(w);  out.w [..., C] weights in the units of PD;  out.pd [...] complex = sum(w) e^{i phi};
%   out.res [...] = ||x e^{-i phi} - A w|| / ||x||;  out.flags [...] int32 (bit 0: iteration cap, bit 1: non-finite pixel, outputs 0);
%   out.atoms the component atoms;  out.info.min_pivot in (0, 1]: 1 = orthogonal components, near 0 = nearly dependent ones.
if nargin < 4 || isempty(mode), mode = 'real'; end
switch mode
    case 'real',  m = 0;
    case 'phase', m = 1;
    otherwise, error('qmri:tissue_fractions:mode', 'mode must be ''real'' or ''phase''');
end
datadims = size(X); s = datadims(end); Npix = prod(datadims(1:end-1));
if s ~= size(dict.D, 2)
    error('qmri:tissue_fractions:size', 'the last dimension of X must equal the columns of dict.D');
end
if size(components, 2) == 1
    atoms = double(components(:));
else
    if size(components, 2) ~= 2
        error('qmri:tissue_fractions:size', 'components must be C x 2 (T1, T2) pairs or a column vector of atom indices');
    end
    lut = double(dict.lut(:, 1:2)); atoms = zeros(size(components, 1), 1);
    for c = 1:size(components, 1)
        d = (lut(:, 1) - double(components(c, 1))).^2 + (lut(:, 2) - double(components(c, 2))).^2;
        [~, atoms(c)] = min(d);                      % the first minimum
    end
end
mrf_dtm_hip(dict, [], []);      % leaves the dictionary set (and checks dict.D)
out.info = qmri_mex('set_components', atoms);
[w, frac, pd, res, flags] = qmri_mex('dict_unmix', complex(double(reshape(X, [Npix, s]))), m);
C = numel(atoms); lead = datadims(1:end-1);
out.w = reshape(w, [lead, C]); out.frac = reshape(frac, [lead, C]);
out.pd = reshape(pd, [lead, 1]); out.res = reshape(res, [lead, 1]); out.flags = reshape(flags, [lead, 1]);
out.atoms = atoms;
end
