function [f, info, trust] = qmri_field_map_estimate(Y, t, varargin)
%QMRI_FIELD_MAP_ESTIMATE  Field map in Hz from multi-echo gradient-echo images, estimated on the GPU (an extension: no reference counterpart).
%   f = qmri_field_map_estimate(Y, t) with Y complex N x M x L (one coil), N x M x C x L or N x M x C x L x S and t the L echo times in
%   seconds (2 <= L <= 8, strictly increasing) returns f, N x M (x S): what qmri_set_field_map takes.  The estimator is the regularised one of
%   Funai, Fessler, Yeo, Olafsson and Noll (IEEE TMI 2008): a penalised cosine fit over all echo pairs and coils with a fixed iteration count.
%   [f, info, trust] = qmri_field_map_estimate(Y, t, 'iters', 200, 'beta', 0.01, 'phase_sign', -1)
%     iters       iterations (default 200; there is no stopping rule)
%     beta        dimensionless smoothness weight (default 0.01)
%     phase_sign  -1 (default): y_l = x .* exp(-1i*2*pi*f*t_l), the sign of the operator of qmri_set_field_map; +1: the other convention
%     info        struct of 1 x S rows: cost0, cost, f_min, f_max, iters, unwrap_limit_hz (= 1 / (2 (t(2) - t(1))): the start wraps beyond it)
%     trust       sum over the echo pairs of the normalised weights, the shape of f: near 0 where there is no signal
%   Example:
%       f = qmri_field_map_estimate(echoes, [0 2e-3 5e-3]);
%       qmri_set_field_map(f, tau);
p = inputParser;
p.addParameter('iters', 0);
p.addParameter('beta', 0);
p.addParameter('phase_sign', -1);
p.parse(varargin{:});
if ~isnumeric(Y) || isreal(Y)
    error('qmri:field_map_estimate:type', 'Y must be complex (the phase between the echoes carries the field)');
end
if ~isreal(t)
    error('qmri:field_map_estimate:t', 't must be real (seconds)');
end
[f, info, trust] = qmri_mex('field_map_estimate', double(Y), double(t(:)), double(p.Results.iters), double(p.Results.beta), double(p.Results.phase_sign));
end
