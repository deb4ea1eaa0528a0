function F = qmri_dict_simulate(alpha, tr, te, t1, t2, params, b1)
% QMRI_DICT_SIMULATE  The fingerprints of a FISP-MRF sequence by extended phase graphs on the GPU (extension, no reference counterpart).
%   The reference loads dictionaries that are already simulated and compressed (SVD_dict_FISP_cut*.mat).  This makes the fingerprints from a
%   flip-angle train; qmri_dict_compress turns them into the fields those files hold:
%
%       [T1, T2] = ndgrid(t1_grid, t2_grid);  T1 = T1.';  T2 = T2.';                 % T2 fastest, as the lut of the reference's files
%       F    = qmri_dict_simulate(alpha, 0.012, 0.002, T1(:), T2(:), struct('nstates', 64));
%       dict = qmri_dict_compress(F, struct('s', 10), [T1(:) T2(:)]);
%
%   alpha: T <= 1024 flip angles in radians; tr, te: seconds, one value or one per frame (te <= tr); t1, t2: K values each, seconds, > 0;
%   b1 (optional): K transmit scales, >= 0.  All real: the pulses rotate about y, the states and the fingerprints stay real.
%   params (optional): struct with nstates (configuration states kept, 1..256, default 32; the truncation is part of the result), inversion
%   (default 1: an inversion pulse before the train), ti (s, default 0), inv_eff (in (0, 1], default 1), single (default 0; 1: F single).
%   F: K x T.  No slice profile, no diffusion, no off-resonance.
if nargin < 6 || isempty(params), params = struct(); end
if nargin < 7, b1 = []; end
if ~isreal(alpha) || ~isreal(t1) || ~isreal(t2) || ~isreal(b1)
    error('qmri:dict_simulate:atoms', 'alpha, t1, t2 and b1 must be real');
end
p = struct();
names = {'nstates', 'inversion', 'ti', 'inv_eff', 'single'};
for k = 1:numel(names)
    if isfield(params, names{k}), p.(names{k}) = double(params.(names{k})); end
end
F = qmri_mex('dict_simulate', double(alpha(:)), double(tr(:)), double(te(:)), double(t1(:)), double(t2(:)), double(b1(:)), p);
end
