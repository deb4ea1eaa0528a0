function out = mrf_dtm_b1_hip(dict, data, par)
% MRF_DTM_B1_HIP  mrf_dtm_hip with a measured B1 map: every pixel is matched against the atoms of its own b1 only.
%   An extension (the reference's mrf_dtm_cpu.m has one flat list of atoms; B1-corrected MRF: Buonincontri & Sawiak 2016, Ma et al. 2017).
%   dict as for mrf_dtm_hip plus  dict.group_ptr (G+1 offsets, 0-based: group g holds rows group_ptr(g)+1 .. group_ptr(g+1) of dict.D)
%   and dict.group_val (G ascending b1 values);  data.X as for mrf_dtm_hip plus  data.B1, one value per pixel (NaN: background, every output 0).
%   Same fields out as mrf_dtm_hip (dm indexes the whole dictionary), plus out.grp (the b1 group of each pixel, 0 = unmatched).
datadims = size(data.X); T = datadims(end); Npix = prod(datadims(1:end-1));
if numel(data.B1) ~= Npix
    error('qmri:mrf_dtm_b1_hip:size', 'data.B1 must hold one value per pixel of data.X');
end
Q = size(dict.lut, 2);
mrf_dtm_hip(dict, [], []);      % leaves the dictionary set (and checks dict.D)
qmri_mex('set_dictionary_groups', double(dict.group_ptr(:)), double(dict.group_val(:)));
X = complex(double(reshape(data.X, [Npix, T])));
if par.f.Xout
    [qmap, pd, mt, dm, grp, xfit] = qmri_mex('dict_match_grouped', X, Q, double(real(data.B1(:))));
else
    [qmap, pd, mt, dm, grp] = qmri_mex('dict_match_grouped', X, Q, double(real(data.B1(:))));
end
if par.f.qout,  out.qmap = reshape(qmap, [datadims(1:end-1), Q]);  out.mask = reshape(grp > 0, [datadims(1:end-1), 1]); end
if par.f.pdout, out.pd = reshape(pd, [datadims(1:end-1), 1]); end
if par.f.mtout, out.mt = reshape(mt, [datadims(1:end-1), 1]); end
if par.f.dmout, out.dm = reshape(single(dm), [datadims(1:end-1), 1]); end
if par.f.Xout,  out.Xfit = reshape(xfit, [datadims(1:end-1), T]);  out.X = data.X; end
if par.f.Yout && isfield(data, 'Y'), out.Y = data.Y; end
out.grp = reshape(grp, [datadims(1:end-1), 1]);
end
