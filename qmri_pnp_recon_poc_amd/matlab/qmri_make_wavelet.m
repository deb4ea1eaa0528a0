function net = qmri_make_wavelet(F, varargin)
% QMRI_MAKE_WAVELET  param.net without a network: joint wavelet soft-thresholding as Step 2 of PnP_ADMM_hip (an extension with no reference
%   counterpart, DESIGN.md section 29).  net = qmri_make_wavelet(F, 'tau', t, 'tau_rel', 0.05, 'levels', 3, 'filter', 'db2', 'joint', true, 'shift', true)
%
%   Step 2 becomes v = Wav_tau(x + uold): the detail coefficients of a periodic orthogonal wavelet transform of the coefficient images are
%   soft-thresholded by tau, jointly over the subspace channels (joint) or each on its own.  It needs no trained weights, is defined for complex
%   TSMIs (param.tsmi_domain = 'complex'; 'real' thresholds real(x + uold)) and fits every F of qmri_make_F / qmri_make_F_traj.  tau: the threshold
%   in the units of the TSMI; empty (default): tau_rel times cmax of the loop's start image, which qmri_mex('wavelet_prox', X0, 0, levels, filter,
%   joint) reports.  levels: 1 .. 4, 2^levels dividing N and M.  filter: 'haar' or 'db2'.  shift: the offsets cycle with the iteration (cycle
%   spinning).  PnP_ADMM_hip sets the step before its loop and clears it afterwards.
if ~isfield(F, 'qmri'), error('qmri:F', 'F must be created by qmri_make_F'); end
o = struct('tau', [], 'tau_rel', 0.05, 'levels', 3, 'filter', 'db2', 'joint', true, 'shift', true);
if mod(numel(varargin), 2), error('qmri:make_wavelet:usage', 'options come in name / value pairs'); end
for k = 1:2:numel(varargin)
    name = char(varargin{k});
    if ~isfield(o, name), error('qmri:make_wavelet:usage', 'unknown option %s', name); end
    o.(name) = varargin{k + 1};
end
if ~(isscalar(o.levels) && any(o.levels == [1 2 3 4])), error('qmri:make_wavelet:levels', 'levels must be 1, 2, 3 or 4'); end
f = find(strcmp(char(o.filter), {'haar', 'db2'}), 1);
if isempty(f), error('qmri:make_wavelet:filter', 'filter must be ''haar'' or ''db2'''); end
if ~isempty(o.tau) && ~(isscalar(o.tau) && isfinite(o.tau) && o.tau >= 0), error('qmri:make_wavelet:tau', 'tau must be finite and >= 0'); end
if ~(isscalar(o.tau_rel) && isfinite(o.tau_rel) && o.tau_rel >= 0), error('qmri:make_wavelet:tau', 'tau_rel must be finite and >= 0'); end
net = struct('qmri_wavelet', true, 'tau', o.tau, 'tau_rel', double(o.tau_rel), 'levels', double(o.levels), 'filter', double(f - 1), ...
             'joint', double(o.joint ~= 0), 'shift', double(o.shift ~= 0));
end
