"""The float64 model of the phase-vocoder stage (include/vorbis_synth_hip.h, "phase vocoder"), steps 1 to 5 with the blocked order of
step 4, and the bound on what a float32 component of the device may differ from it by.

The model reads the float32 rows the device reads and does the same IEEE operations in the same order, so only three things can
differ between the two: the two libraries' atan2 and sin / cos (a few units in the last place each), the roundings that follow
them (an operation whose operands differ in the last place can round either way), and the one rounding to float32 at the end.

bound() adds these up, per component of out[t][k], U = 2^-52 being the spacing of float64 at 1:

  e_A    = 7 * 2^-51        one angle. |A| <= pi < 4, so a unit in its last place is at most 2^-51; numpy's atan2 is within 1 of them
                            and the device library's within 6 (the OpenCL bound its double atan2 is built to).
  P_k    = phi_k + 2 pi     bounds |d|: two angles apart by at most 2 pi, less phi_k.
  e_inc  = 2 e_A + U (3 P_k + 3 pi) + 2^-51
                            one inc_t: the two angles; the roundings of A1 - A0 (at most 2 pi), of "- phi" and of "phi +" (at most
                            P_k each), of the wrapped difference (at most pi) and of the product 2 pi * rint (at most P_k, and only
                            where the two rint disagree); and 2^-51 for the representation error of 2 pi, 2.5e-16, which enters
                            once per step when a d / (2 pi) on a tie rounds to the other side in one of the two and moves the phase
                            by one turn of the DOUBLE 2 pi instead of none.
  a_t    = pi + t P_k       bounds |acc_u| for u <= t, and every block sum and carry on the way to it.
  e_acc  = e_A + t e_inc + (t + t / 64 + 2) U a_t
                            acc_t: A[0], t increments, and the rounding of each of the additions that lead to it in the blocked
                            order (at most t inside blocks and sums, t / 64 + 1 carries), each at most U |result|.
  e_out  = m (e_acc + 8 U) + 2^-24 (|v| + m (e_acc + 8 U)) + 2^-149
                            the argument error of sin / cos times m, 8 U for the two libraries' sin / cos and the product, and the
                            rounding of the device's float64 value to float32: half a unit in the last place of a float32 is at most
                            2^-24 of the value (2^-149: a subnormal result). m is bit-equal on both sides (sqrt, products and sums
                            are correctly rounded in both) and v = m cos(acc) or m sin(acc) is the model's unrounded float64 value,
                            which is what the device's float32 is compared with.

The last term dominates by four or more orders of magnitude at the sizes the tests use, and it is tight: a correctly rounded
float32 reaches half a unit in the last place, so over 10^5 components the worst |d| / bound comes out just below 1 by construction
and says little; what the phase terms leave room for is visible only in a component whose rounding happens to be small. The
tests therefore also report the worst |d| / (2^-24 |v|) - 1 excess, which must stay within the phase terms alone."""
import numpy as np

BLOCK = 64
TWO_PI = 2.0 * np.pi
U = 2.0 ** -52


def num_rows(F, rate):
    """ceil(F / rate) in float64."""
    return int(np.ceil(np.float64(F) / np.float64(rate)))


def num_samples(T, rate):
    return int(round(T / rate))


def phi_advance(n_fft, hop):
    val = 1.0 / (n_fft * (1.0 / TWO_PI))
    return hop * (np.arange(n_fft // 2 + 1) * val)


def polar(X):
    """A and G of step 2 from complex64 rows: float64 atan2 with C99's signed zeros (numpy's arctan2 has them) and sqrt(re^2 + im^2)."""
    X = np.asarray(X, np.complex64)
    re, im = X.real.astype(np.float64), X.imag.astype(np.float64)
    return np.arctan2(im, re), np.sqrt(re * re + im * im)


def positions(F, rate):
    t = np.arange(num_rows(F, rate), dtype=np.float64)
    s = t * np.float64(rate)
    i = np.floor(s)
    return i.astype(np.int64), s - i


def increments(A, F, rate, phi):
    """inc_t [F_out][nb] of step 3; A is padded with the angle of +0 + 0i behind row F - 1."""
    i, _ = positions(F, rate)
    Ap = np.concatenate([A, np.zeros((2 + max(0, int(i.max(initial=0)) + 2 - F), A.shape[1]))])
    d = Ap[i + 1] - Ap[i] - phi
    return phi + (d - TWO_PI * np.rint(d / TWO_PI))


def accumulate(A0, inc):
    """acc_t [F_out][nb] in the blocked order of step 4."""
    n = inc.shape[0]
    acc = np.empty_like(inc)
    carry = A0.copy()
    for b0 in range(0, n, BLOCK):
        blk = inc[b0:b0 + BLOCK]
        a = carry.copy()
        s = np.zeros_like(carry)
        for u in range(blk.shape[0]):
            acc[b0 + u] = a
            a = a + blk[u]
            s = s + blk[u]
        carry = carry + s
    return acc


def vocoder(X, rate, n_fft, hop):
    """Steps 1 to 5 on one segment's complex64 rows [F][nb]: (the unrounded float64 values re, im [F_out][nb], the bound on each
    component [F_out][nb])."""
    X = np.asarray(X, np.complex64).reshape(-1, n_fft // 2 + 1)
    F, nb = X.shape
    n = num_rows(F, rate)
    if n == 0:
        z = np.zeros((0, nb))
        return z, z, z
    A, G = polar(X)
    phi = phi_advance(n_fft, hop)
    i, alpha = positions(F, rate)
    with np.errstate(invalid="ignore", over="ignore"):
        inc = increments(A, F, rate, phi)
        acc = accumulate(A[0], inc)
        Gp = np.concatenate([G, np.zeros((2 + max(0, int(i.max()) + 2 - F), nb))])
        m = (1.0 - alpha)[:, None] * Gp[i] + alpha[:, None] * Gp[i + 1]
        re, im = m * np.cos(acc), m * np.sin(acc)
    return re, im, (m, phi)


def bound(v, m, phi):
    """The bound on |device float32 - v| for the unrounded model value v [F_out][nb] (see the module's docstring)."""
    t = np.arange(v.shape[0], dtype=np.float64)[:, None]
    e_A = 7.0 * 2.0 ** -51
    P = phi[None, :] + TWO_PI
    e_inc = 2.0 * e_A + U * (3.0 * P + 3.0 * np.pi) + 2.0 ** -51
    a_t = np.pi + t * P
    e_acc = e_A + t * e_inc + (t + t / BLOCK + 2.0) * U * a_t
    e = m * (e_acc + 8.0 * U)
    return e + 2.0 ** -24 * (np.abs(v) + e) + 2.0 ** -149


def phase_part(v, m, phi):
    """The part of bound() that is not the final rounding: what |d| may exceed half a float32 unit of v by."""
    return bound(v, m, phi) - 2.0 ** -24 * np.abs(v)


def check(got, X, rate, n_fft, hop, what=None):
    """A device segment (complex64 [F_out][nb]) against the model under the bound; returns (worst |d| / bound, worst (|d| - 2^-24
    |v|) / phase part), the second at most 1 wherever the first is."""
    re, im, (m, phi) = vocoder(X, rate, n_fft, hop)
    got = np.asarray(got, np.complex64).reshape(re.shape)
    worst, worst_phase = 0.0, 0.0
    for v, g in ((re, got.real), (im, got.imag)):
        if v.size == 0:
            continue
        assert np.isfinite(g).all(), what
        d = np.abs(g.astype(np.float64) - v)
        b = bound(v, m, phi)
        assert (d <= b).all(), (what, float((d / b).max()))
        worst = max(worst, float((d / b).max()))
        worst_phase = max(worst_phase, float(((d - 2.0 ** -24 * np.abs(v)) / phase_part(v, m, phi)).max()))
    return worst, worst_phase


def librosa_loop(X, rate, n_fft, hop):
    """A literal transcription of librosa.phase_vocoder's sequential loop on D = X.T (complex128 out, time last there, first here)."""
    D = np.asarray(X, np.complex64).astype(np.complex128).T  # [nb][F]
    time_steps = np.arange(0, D.shape[-1], rate, dtype=np.float64)
    shape = list(D.shape)
    shape[-1] = len(time_steps)
    d_stretch = np.zeros(shape, dtype=np.complex128)
    phi_adv = phi_advance(n_fft, hop)
    if D.shape[-1] == 0:
        return d_stretch.T
    phase_acc = np.angle(D[..., 0])
    padding = [(0, 0) for _ in D.shape]
    padding[-1] = (0, 2)
    D = np.pad(D, padding, mode="constant")
    for t, step in enumerate(time_steps):
        columns = D[..., int(step):int(step + 2)]
        alpha = np.mod(step, 1.0)
        mag = (1.0 - alpha) * np.abs(columns[..., 0]) + alpha * np.abs(columns[..., 1])
        d_stretch[..., t] = mag * (np.cos(phase_acc) + 1j * np.sin(phase_acc))
        dphase = np.angle(columns[..., 1]) - np.angle(columns[..., 0]) - phi_adv
        dphase = dphase - 2.0 * np.pi * np.round(dphase / (2.0 * np.pi))
        phase_acc += phi_adv + dphase
    return d_stretch.T


def reorder_bound(F_out, m, phi):
    """What the model's unrounded values may differ from librosa_loop's by, per component [F_out][nb]: both do the same float64
    operations on the same angles, but the loop adds inc_t one after another and the model in blocks. A sum of t terms each at most
    a_t in magnitude differs between two orders by at most 2 t U a_t (t roundings of at most U a_t / 2 in each); the argument of
    sin / cos moves by that, the value by m times it. Added: 4 U m for numpy's abs (hypot) against sqrt(re^2 + im^2), and the
    arange position against t * rate, which agree to a unit in the last place of s_t: (alpha's change) times the magnitudes' span is
    covered by 2^-40 m at these sizes (s_t < 2^12: one unit is 2^-41)."""
    t = np.arange(F_out, dtype=np.float64)[:, None]
    a_t = np.pi + t * (phi[None, :] + TWO_PI)
    return m * (2.0 * t * U * a_t + 4.0 * U) + 2.0 ** -40 * m + 1e-300


def random_rows(rng, F, n_fft):
    nb = n_fft // 2 + 1
    return (rng.standard_normal((F, nb)) + 1j * rng.standard_normal((F, nb))).astype(np.complex64)
