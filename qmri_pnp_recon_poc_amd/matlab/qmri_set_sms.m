function qmri_set_sms(E)
% QMRI_SET_SMS  Attach the phases of a simultaneous multi-slice (SMS) acquisition to the operator (extension, no reference counterpart).
%   Z slices excited together add up in every coil, slice b under the known phase E(t, b) in frame t (RF phase cycling):
%
%       F = qmri_make_F(...);                                              % or qmri_make_F_traj: the operator of ONE slice
%       Z = 2;  t = (0:T-1)';
%       qmri_set_sms(exp(2i*pi * mod(t, Z) * (0:Z-1) / Z));                % E: T x Z complex, here the CAIPI cycle E(t,b) = exp(2*pi*i*b*mod(t,Z)/Z)
%       X = PnP_ADMM_sms_hip(Y, maps, param);                              % the Z slices of every group, solved jointly
%       qmri_set_sms([]);                                                  % clears the phases
%
%   1 <= Z <= 8, every value finite, any modulus.  The phases belong to the operator: making a new one (qmri_make_F, qmri_make_F_traj) drops them,
%   as it drops the sample weights; an operator with a field map attached refuses them (one map cannot serve Z slices).  No other call reads them.
if isempty(E), qmri_mex('set_sms', []); return; end
qmri_mex('set_sms', complex(double(E)));
end
