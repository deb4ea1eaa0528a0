function [F, dF, crb, flags] = qmri_dict_simulate_grad(alpha, tr, te, t1, t2, params, b1, V)
% QMRI_DICT_SIMULATE_GRAD  The fingerprints of qmri_dict_simulate with their derivatives and the Cramer-Rao bound they give, in one GPU launch
%   (extension, no reference counterpart).  Forward-mode differentiation of the extended-phase-graph recursion, exact to rounding:
%
%       [F, dF, crb, flags] = qmri_dict_simulate_grad(alpha, 0.012, 0.002, T1(:), T2(:), struct('nstates', 64), [], dict.V);
%       std_t1 = sigma * sqrt(crb(idx, 2)) ./ abs(pd);            % per pixel: idx the matched atom, pd its proton density, sigma the noise level
%
%   alpha, tr, te, t1, t2, b1: as in qmri_dict_simulate.  params (optional): its fields, plus nparams (2, the default: derivatives with respect to
%   T1 and T2; 3: b1 as well) and bound_only (default 0; 1: only crb and flags are computed, F and dF come back empty and no K x T array is made).
%   V (optional): a real T x s subspace, s <= 16 (the V of qmri_dict_compress): the bound is that of the compressed fingerprints.
%   F: K x T, the bits of qmri_dict_simulate.  dF: K x T x P.  crb: K x (1 + P), column 1 the proton density's, then T1, T2 (, b1): a pixel
%   rho * atom k + noise of standard deviation sigma per real and imaginary part and channel has std(theta_q) >= sigma sqrt(crb(k, 1 + q)) / |rho|
%   and std(real(rho)) >= sigma sqrt(crb(k, 1)).  flags: int32 K x 1, 1 where the Fisher matrix is singular (crb is Inf there; s < 1 + P always is).
%   dF is computed when two outputs are asked for, the bound when three are.  No slice profile.
if nargin < 6 || isempty(params), params = struct(); end
if nargin < 7, b1 = []; end
if nargin < 8, V = []; end
if ~isreal(alpha) || ~isreal(t1) || ~isreal(t2) || ~isreal(b1) || ~isreal(V)
    error('qmri:dict_simulate_grad:atoms', 'alpha, t1, t2, b1 and V must be real');
end
p = struct();
names = {'nstates', 'inversion', 'ti', 'inv_eff', 'single', 'nparams', 'bound_only'};
for k = 1:numel(names)
    if isfield(params, names{k}), p.(names{k}) = double(params.(names{k})); end
end
[F, dF, crb, flags] = qmri_mex('dict_simulate_grad', double(alpha(:)), double(tr(:)), double(te(:)), double(t1(:)), double(t2(:)), double(b1(:)), p, double(V));
crb = crb.';
end
