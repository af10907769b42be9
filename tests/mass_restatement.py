"""numpy restatement of Hamiltonian_mass (barlib/src/HMC_mass.cc:315-368), loop for loop where the order matters.

Built on the CPU oracle's likelihood_grad_log_like, measure_spectrum and Lag2Eul.  One deliberate deviation from
upstream, shared with the engine: for mass_type 2 the corner mode (N/2, N/2, N/2), whose bin index is N_bin, reads an
empty bin (0) where upstream reads likeli_power[N_bin], one past the end of the array (HMC_mass.cc:79); that is how
measure_spectrum itself treats the mode (field_statistics.cpp:50-53).
"""
import numpy as np

MASS_F_TYPES = (1, 2, 3, 4, 5)
MASS_R_TYPES = (0, 5, 6, 60)


def inv_ps(signal_PS):
    """inv_ps (117-124) over the whole grid: 1/P where P > 0, else 0."""
    P = np.asarray(signal_PS, dtype=np.float64).ravel()
    out = np.zeros_like(P)
    np.divide(1.0, P, out=out, where=P > 0.0)
    return out


def k_axis(n, L):
    """calc_ki (scale_space.cpp:41-51)."""
    kfac = 2.0 * np.pi / L
    i = np.arange(n)
    return np.where(i <= n // 2, kfac * i.astype(np.float64), -kfac * (n - i).astype(np.float64))


def k_abs(n, L):
    """|k| of every full-grid cell (k_squared's folding, scale_space.cpp:16-38), kx*kx + ky*ky + kz*kz in that order."""
    k = k_axis(n, L)
    k2 = k * k
    return np.sqrt((k2[:, None, None] + k2[None, :, None]) + k2[None, None, :]).ravel()


def spectrum_dk(n, L, n_bin):
    """measure_spectrum's bin width (field_statistics.cpp:37-39)."""
    knyq = (2.0 * np.pi / L) * float(n // 2)
    return np.sqrt(knyq * knyq + knyq * knyq + knyq * knyq) / float(n_bin)


def force_bins(n, L, n_bin):
    """(ULONG)(|k| / dk) of every full-grid cell (74-76); -1 marks k = 0, which gets 0 (78-81)."""
    kr = k_abs(n, L)
    b = np.floor(kr / spectrum_dk(n, L, n_bin)).astype(np.int64)
    return np.where(kr > 0.0, b, -1)


def force_power(orc, signal, n_bin):
    """likeli_force_power (39-50): measure_spectrum of likelihood_grad_log_like(signal) -> (kmode, power)."""
    return orc.measure_spectrum(orc.likelihood_grad_log_like(signal), n_bin)


def likeli_force_mass(p, signal_PS, power):
    """Hamiltonian_mass_likeli_force (53-83) + likeli_force_mass (127-142), before mass_factor."""
    n_bin = len(power)
    b = force_bins(p.Nx, p.L, n_bin)
    Pf = np.zeros(b.size)
    ok = (b >= 0) & (b < n_bin)  # b == n_bin: the corner mode, an empty bin
    Pf[ok] = np.asarray(power)[b[ok]]
    invP = inv_ps(signal_PS)
    return 2 * invP + np.sqrt(invP * Pf)


def likeli_force_mass_loop(p, signal_PS, power):
    """Lines 53-83 and 127-142 as written: a triple loop over the full grid, one cell at a time."""
    n, L, n_bin = p.Nx, p.L, len(power)
    kfac = 2.0 * np.pi / L
    knyq = kfac * float(n // 2)
    dk = np.sqrt(knyq * knyq + knyq * knyq + knyq * knyq) / float(n_bin)
    P = np.asarray(signal_PS, dtype=np.float64).ravel()
    out = np.zeros(n ** 3)
    for i in range(n):
        kx = kfac * i if i <= n // 2 else -kfac * (n - i)
        for j in range(n):
            ky = kfac * j if j <= n // 2 else -kfac * (n - j)
            for k in range(n):
                kz = kfac * k if k <= n // 2 else -kfac * (n - k)
                l = k + n * (j + n * i)
                kr = np.sqrt(kx * kx + ky * ky + kz * kz)
                nbin = int(kr / dk)
                pf = 0.0
                if kr > 0.0 and nbin < n_bin:  # nbin == n_bin only for the corner mode: the deliberate deviation
                    pf = power[nbin]
                invP = 1.0 / P[l] if P[l] > 0.0 else 0.0
                out[l] = 2 * invP + np.sqrt(invP * pf)
    return out


def mean_likeli_force(p, kmode, power):
    """Hamiltonian_mass_mean_likeli_force (86-114): sum_b 4 pi k_b^2 dk P_b / sum_b 4 pi k_b^2 dk."""
    n_bin = len(power)
    dk = spectrum_dk(p.Nx, p.L, n_bin)
    fm = kv = 0.0
    for i in range(n_bin):
        fm += 4. * np.pi * float(kmode[i]) * float(kmode[i]) * dk * float(power[i])
    for i in range(n_bin):
        kv += 4. * np.pi * float(kmode[i]) * float(kmode[i]) * dk
    return fm / kv


def pacman_difference(d, L):
    """pacman.cpp:42-47, sign quirk kept: d > L/2 becomes L - d."""
    d = np.where(d > L / 2, L - d, d)
    return np.where(d < -(L / 2), L + d, d)


def wprime_il(p, px, py, pz, l):
    """Wprime_il (179-227): the SPH-kernel gradient between every particle i and the centre of cell l.
    Returns (W'x, W'y, W'z, q < 2)."""
    n, L = p.Nx, p.L
    d = L / n
    xl, yl, zl = ((l // n // n) + 0.5) * d, ((l // n) % n + 0.5) * d, (l % n + 0.5) * d
    h = p.particle_kernel_h
    h2 = h * h
    norm = 1. / (np.pi * (h2 * h2 * h))  # gsl_pow_5
    dx, dy, dz = pacman_difference(px - xl, L), pacman_difference(py - yl, L), pacman_difference(pz - zl, L)
    q = np.sqrt(dx * dx + dy * dy + dz * dz) / h
    with np.errstate(divide="ignore", invalid="ignore"):
        common = np.where(q >= 1, norm * (3 - 0.75 * q - 3. / q), norm * (2.25 * q - 3))
    common = np.where(q >= 2, 0.0, common)
    return dx * common, dy * common, dz * common, q < 2


def grad_inv_lap_FS(n, L, A, index):
    """gradient.cpp:157-211 on a half-complex array: -i k_index / k^2, 0 at k = 0 and on every Nyquist plane."""
    k = k_axis(n, L)
    KX, KY, KZ = k[:, None, None], k[None, :, None], k[None, None, : n // 2 + 1]
    kmod = (KX * KX + KY * KY) + KZ * KZ
    fac = np.where(kmod > 0, 1 / np.where(kmod > 0, kmod, 1.0), 0.0)
    ki = (KX, KY, KZ)[index - 1] * fac
    out = np.empty_like(A)
    out.real = ki * A.imag
    out.imag = -(ki * A.real)
    i = np.arange(n)
    nyq = (i[:, None, None] == n // 2) | (i[None, :, None] == n // 2) | (np.arange(n // 2 + 1)[None, None, :] == n // 2)
    out[np.broadcast_to(nyq, out.shape)] = 0.0
    return out


def jasche_literal(p, px, py, pz, window, noise):
    """likeli_force_1st_order_diagonal_mass (268-305) as written: per cell l with window[l] > 0, three R2C, the inverse
    Laplacian gradients, one C2R (normalised, fftwrapper.cc:44-45) and the weighted square at the OUTPUT index i."""
    n = p.Nx
    N = n ** 3
    shape = (n, n, n)
    window, noise = np.asarray(window).ravel(), np.asarray(noise).ravel()
    mass_r = np.zeros(N)
    for l in range(N):
        if window[l] > 0:
            wx, wy, wz, _ = wprime_il(p, px, py, pz, l)
            C = grad_inv_lap_FS(n, p.L, np.fft.rfftn(wx.reshape(shape)), 1)
            C = C + grad_inv_lap_FS(n, p.L, np.fft.rfftn(wy.reshape(shape)), 2)
            C = C + grad_inv_lap_FS(n, p.L, np.fft.rfftn(wz.reshape(shape)), 3)
            D = np.fft.irfftn(C, s=shape, axes=(0, 1, 2)).ravel()
            mass_r += window * (D / noise) ** 2
    m = p.rho_c * (p.L * p.L * p.L) / N
    return (m * m) * mass_r


def glap_impulse_fields(n, L):
    """G_j = C2R[grad_inv_lap_FS_j(1)] / N: D_l's response to a unit W' at particle 0."""
    ones = np.ones((n, n, n // 2 + 1), dtype=np.complex128)
    return [np.fft.irfftn(grad_inv_lap_FS(n, L, ones, j), s=(n, n, n), axes=(0, 1, 2)).ravel() for j in (1, 2, 3)]


def jasche_D_convolution(p, px, py, pz, l, G):
    """D_l by linearity: sum over the particles within 2h of cell l of sum_j W'_ij G_j[(i' - i) mod n]."""
    n = p.Nx
    wx, wy, wz, near = wprime_il(p, px, py, pz, l)
    i = np.nonzero(near)[0]
    I = np.arange(n ** 3)
    X, Y, Z = I // (n * n), (I // n) % n, I % n
    gi = (((X[None, :] - (i // (n * n))[:, None]) % n) * n + ((Y[None, :] - ((i // n) % n)[:, None]) % n)) * n \
        + ((Z[None, :] - (i % n)[:, None]) % n)
    return (wx[i][:, None] * G[0][gi] + wy[i][:, None] * G[1][gi] + wz[i][:, None] * G[2][gi]).sum(axis=0)


def jasche_convolution(p, px, py, pz, window, noise):
    """The engine's form of the Jasche diagonal: the G convolution, no FFT per cell."""
    n = p.Nx
    N = n ** 3
    window, noise = np.asarray(window).ravel(), np.asarray(noise).ravel()
    G = glap_impulse_fields(n, p.L)
    acc = np.zeros(N)
    for l in range(N):
        if window[l] > 0:
            acc += jasche_D_convolution(p, px, py, pz, l, G) ** 2
    m = p.rho_c * (p.L * p.L * p.L) / N
    return (m * m) * (window * (acc / (noise * noise)))


def hamiltonian_mass(p, orc, signal, signal_PS, window, noise, n_bin=200, mass_factor=1.0, iGibbs=1, s_eps_total=0):
    """Hamiltonian_mass (315-368) for p.mass_type -> (mass_f, mass_r), None where the type has none.  ``orc`` is an
    oracle context loaded with the case's arrays."""
    t = p.mass_type
    mass_f = mass_r = None
    jasche = t in (5, 6) or (t == 60 and not iGibbs < s_eps_total)
    if t in (2, 3):
        kmode, power = force_power(orc, signal, n_bin)
        if t == 2:
            mass_f = likeli_force_mass(p, signal_PS, power)
        else:
            invP = inv_ps(signal_PS)
            mass_f = 2 * invP + np.sqrt(invP * mean_likeli_force(p, kmode, power))
    elif t in (1, 5):
        mass_f = inv_ps(signal_PS)
    elif t == 4:
        mass_f = np.asarray(signal_PS, dtype=np.float64).ravel().copy()
    if t in MASS_R_TYPES:
        if jasche:
            _, px, py, pz = orc.Lag2Eul(signal)  # as configured, no deltaQ_factor (242-257)
            mass_r = jasche_literal(p, px, py, pz, window, noise)
        else:
            mass_r = np.ones(p.N)
    if mass_f is not None:
        mass_f = mass_factor * mass_f
    return mass_f, mass_r
