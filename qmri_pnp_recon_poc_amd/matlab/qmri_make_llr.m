function net = qmri_make_llr(F, varargin)
% QMRI_MAKE_LLR  param.net without a network: the locally low-rank (LLR) regulariser as Step 2 of PnP_ADMM_hip (an extension with no reference
%   counterpart, DESIGN.md section 25).  net = qmri_make_llr(F, 'tau', t, 'tau_rel', 0.02, 'block', 8, 'shift', true)
%
%   Step 2 becomes v = LLR_tau(x + uold): the singular values of every block x block patch of the coefficient images are soft-thresholded by tau.
%   It needs no trained weights, is defined for complex TSMIs (param.tsmi_domain = 'complex'; 'real' thresholds real(x + uold)) and fits every F of
%   qmri_make_F / qmri_make_F_traj.  tau: the threshold in the units of the TSMI; empty (default): tau_rel times sigma_max of the loop's start
%   image, which qmri_mex('llr_prox', X0, 0, block) reports.  block: 4, 8 or 16, dividing N and M.  shift: the block offsets cycle with the iteration.
%   PnP_ADMM_hip sets the step before its loop and clears it afterwards.
if ~isfield(F, 'qmri'), error('qmri:F', 'F must be created by qmri_make_F'); end
o = struct('tau', [], 'tau_rel', 0.02, 'block', 8, 'shift', true);
if mod(numel(varargin), 2), error('qmri:make_llr:usage', 'options come in name / value pairs'); end
for k = 1:2:numel(varargin)
    name = char(varargin{k});
    if ~isfield(o, name), error('qmri:make_llr:usage', 'unknown option %s', name); end
    o.(name) = varargin{k + 1};
end
if ~any(o.block == [4 8 16]), error('qmri:make_llr:block', 'block must be 4, 8 or 16'); end
if ~isempty(o.tau) && ~(isscalar(o.tau) && isfinite(o.tau) && o.tau >= 0), error('qmri:make_llr:tau', 'tau must be finite and >= 0'); end
if ~(isscalar(o.tau_rel) && isfinite(o.tau_rel) && o.tau_rel >= 0), error('qmri:make_llr:tau', 'tau_rel must be finite and >= 0'); end
net = struct('qmri_llr', true, 'tau', o.tau, 'tau_rel', double(o.tau_rel), 'block', double(o.block), 'shift', double(o.shift ~= 0));
end
