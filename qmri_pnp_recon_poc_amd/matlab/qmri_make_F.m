function F = qmri_make_F(pattern, N, M, rate, V)
% QMRI_MAKE_F  GPU forward/adjoint operator with the reference's plugin surface.
%   Replaces main_recon_tsmis_FFT.m:220-229:
%       [P] = setup_subsampling_spiralgrided(N,M,spiral_sampling_curve,V);   (or setup_subsampling_epi)
%       F.forward = @(x) P.for(reshape(fft2(x),[],1))/sqrt(N*M);
%       F.adjoint = @(x) (ifft2(reshape(P.adj(x),N,M,[]))*sqrt(N*M));
%   by   F = qmri_make_F('Spiral', N, M, spiral_sampling_curve, V);          (or 'EPI', ..., epi_sampling_rate, V)
%   N, M in {32 64 96 112 128 160 192 224 256}, chosen independently (EPI); the spiral is square, N == M.
%   F = qmri_make_F('SpiralExact', N, N, spiral_sampling_curve, V) keeps the spiral's samples at their exact positions (no rounding onto the
%   grid): a NUFFT operator (DESIGN.md section 14).  For a measured trajectory see qmri_make_F_traj.
T = size(V, 1);  s = size(V, 2);
if strcmp(pattern, 'SpiralExact')
    if N ~= M, error('qmri:pattern', 'the spiral is square (setup_subsampling_spiralgrided.m:28-31): N must equal M'); end
    [fp, omega] = qmri_mex('build_spiral_traj', N, rate, T);
    F = qmri_make_F_traj(N, M, V, fp, omega);
    return
end
switch pattern
    case 'Spiral'
        if N ~= M, error('qmri:pattern', 'the spiral mask is square (setup_subsampling_spiralgrided.m:28-31): N must equal M'); end
        [fp, k] = qmri_mex('build_spiral', N, rate, T);
    case 'EPI',    [fp, k] = qmri_mex('build_epi', N, M, rate, T);
    otherwise, error('qmri:pattern', 'unknown subsampling pattern %s', pattern);
end
qmri_mex('set_operator', N, M, real(double(V)), fp, k);
F.forward = @(x) qmri_mex('forward', double(x));
F.adjoint = @(y) qmri_mex('adjoint', complex(double(y)), [N M s]);
F.qmri = struct('N', N, 'M', M, 's', s);      % marks F as GPU resident for PnP_ADMM_hip
end
