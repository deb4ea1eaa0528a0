function F = qmri_dict_simulate_seq(alpha, tr, te, t1, t2, blocks, ncycles, params, b1)
% QMRI_DICT_SIMULATE_SEQ  EPG fingerprints of a prepared, repeated FISP train on the GPU (extension, no reference counterpart).
%   qmri_dict_simulate describes one experiment: equilibrium, at most one inversion, one uninterrupted train.  Here the train is cut into blocks;
%   in front of its frames a block waits (free relaxation), then plays a preparation; the block list is played ncycles times from equilibrium and
%   the last cycle is recorded -- repeated trains (3-D, multi-slice, SMS MRF) and cardiac MRF with its per-heartbeat preparations and RR waits.
%
%       blocks = struct('nframes', {12, 12, 12, 12}, 'prep', {'inversion', 'none', 't2', 't2'}, 'wait', {0, 0.83, 0.79, 0.75}, ...
%                       'prep_time', {0.021, 0, 0.040, 0.080});
%       F    = qmri_dict_simulate_seq(alpha, 0.012, 0.002, T1(:), T2(:), blocks, 1, struct('nstates', 64));
%       dict = qmri_dict_compress(F, struct('s', 10), [T1(:) T2(:)]);
%
%   alpha, tr, te, t1, t2, b1: as in qmri_dict_simulate.  blocks: a struct array, 1 to 64 elements, with the fields nframes (frames of the block;
%   they sum to numel(alpha)), prep ('none', 'inversion' or 't2', or 0, 1, 2; default 'none'), wait (s in front of the preparation; default 0),
%   prep_time (s: TI of an inversion, echo time of a T2 preparation; default 0) and prep_eff (inversion efficiency / T2-preparation scale in
%   (0, 1]; default 1).  The preparations are idealised (a crusher follows; T1 during a T2 preparation is neglected) and not scaled by b1.
%   ncycles: 1 to 16 (default 1).  params: the fields nstates (32) and single (0) of qmri_dict_simulate; inversions are stated in the blocks.
%   F: K x T.  One block of all frames with an inversion (or none) and ncycles = 1 gives qmri_dict_simulate's numbers.
if nargin < 7 || isempty(ncycles), ncycles = 1; end
if nargin < 8 || isempty(params), params = struct(); end
if nargin < 9, b1 = []; end
if ~isreal(alpha) || ~isreal(t1) || ~isreal(t2) || ~isreal(b1)
    error('qmri:dict_simulate_seq:atoms', 'alpha, t1, t2 and b1 must be real');
end
if ~isstruct(blocks) || ~isfield(blocks, 'nframes') || numel(blocks) < 1 || numel(blocks) > 64
    error('qmri:dict_simulate_seq:blocks', 'blocks must be a struct array of 1 to 64 elements with the field nframes');
end
kinds = {'none', 'inversion', 't2'};
B = zeros(5, numel(blocks));
for k = 1:numel(blocks)
    b = blocks(k);
    prep = 0;
    if isfield(b, 'prep') && ~isempty(b.prep)
        if ischar(b.prep) || isstring(b.prep)
            prep = find(strcmp(char(b.prep), kinds)) - 1;
            if isempty(prep)
                error('qmri:dict_simulate_seq:blocks', 'blocks(%d).prep must be ''none'', ''inversion'' or ''t2''', k);
            end
        else
            prep = double(b.prep);
        end
    end
    B(:, k) = [double(b.nframes); prep; field_or(b, 'wait', 0); field_or(b, 'prep_time', 0); field_or(b, 'prep_eff', 1)];
end
p = struct();
names = {'nstates', 'single'};
for k = 1:numel(names)
    if isfield(params, names{k}), p.(names{k}) = double(params.(names{k})); end
end
F = qmri_mex('dict_simulate_seq', double(alpha(:)), double(tr(:)), double(te(:)), double(t1(:)), double(t2(:)), double(b1(:)), p, B, double(ncycles));
end

function v = field_or(s, name, dflt)
v = dflt;
if isfield(s, name) && ~isempty(s.(name)), v = double(s.(name)); end
end
