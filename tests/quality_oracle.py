"""Float64 NumPy statement of the objective quality measures: LLR, LPC cepstral distance, Klatt's weighted spectral
slope (WSS) and the frequency-weighted segmental SNR (fwSNRseg), as restated from Loizou's comp_llr.m, comp_cep.m, comp_wss.m and
comp_fwseg.m (Speech Enhancement: Theory and Practice, §11.1-11.2).

Test infrastructure: the yardstick of ssr_quality_metrics, written from the definitions with plain loops where order matters.
x is the target (clean), y the estimate; both are widened to float64 and EPS is added to every sample.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
LLR_CLIP, CEP_CLIP = 2.0, 10.0
FW_LO, FW_HI = -10.0, 35.0
NAMES = ("llr", "cep_dist", "wss", "fwseg_snr")

CENT = np.array([50, 120, 190, 260, 330, 400, 470, 540, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54,
                 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63])
BW = np.array([70.0] * 7 + [77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457, 199.776,
                            217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136])


def frame_geometry(fs, n):
    """-> (L, R, M): frame length (30 ms rounded half up), hop L // 4, frames max(0, (n - L) // R) - the framing of §10."""
    L = (3 * int(fs) + 50) // 100
    R = L // 4
    M = max(0, (int(n) - L) // R) if R > 0 else 0
    return L, R, M


def nfft(fs):
    L = frame_geometry(fs, 0)[0]
    return int(2 ** int(np.ceil(np.log2(2 * L))))


def default_order(fs):
    return 10 if fs < 10000 else 16


def window(L):
    return 0.5 * (1 - np.cos(2 * np.pi * np.arange(1, L + 1) / (L + 1)))


def trim_count(M):
    return int(np.floor(0.95 * M + 0.5))


def trimmed_mean(v):
    v = np.asarray(v, np.float64)
    return float(np.mean(np.sort(v)[:trim_count(len(v))]))


def filters(fs):
    """[25, N/2] float64 critical-band filters of comp_wss.m / comp_fwseg.m."""
    N = nfft(fs)
    half = fs / 2.0
    j = np.arange(N // 2, dtype=np.float64)
    thr = np.exp(-30.0 / (2.0 * 2.303))
    W = np.zeros((25, N // 2))
    for b in range(25):
        f0 = CENT[b] / half * (N // 2)
        bwb = BW[b] / half * (N // 2)
        u = (j - np.floor(f0)) / bwb
        w = np.exp(-11.0 * (u * u) + np.log(BW[0]) - np.log(BW[b]))
        W[b] = np.where(w > thr, w, 0.0)
    return W


def frames(s, fs):
    L, R, M = frame_geometry(fs, len(s))
    w = window(L)
    return [w * s[j * R:j * R + L] for j in range(M)]


# ---- LPC --------------------------------------------------------------------------------------------------------------------
def lags(f, P):
    L = len(f)
    return np.array([np.dot(f[:L - k], f[k:]) for k in range(P + 1)])


def levinson(r, P):
    """-> a = [1, -alpha_1, .., -alpha_P]; the recursion stops where E_{i-1} is not finite and positive (higher orders stay 0)."""
    alpha = np.zeros(P + 1)
    E = r[0]
    for i in range(1, P + 1):
        if not (np.isfinite(E) and E > 0):
            break
        acc = r[i]
        for m in range(1, i):
            acc -= alpha[m] * r[i - m]
        k = acc / E
        prev = alpha.copy()
        for m in range(1, i):
            alpha[m] = prev[m] - k * prev[i - m]
        alpha[i] = k
        E = (1 - k * k) * E
    a = -alpha
    a[0] = 1.0
    return a


def toeplitz(r):
    P = len(r) - 1
    return np.array([[r[abs(i - j)] for j in range(P + 1)] for i in range(P + 1)])


def llr_frame(rx, ax, ay):
    T = toeplitz(rx)
    num, den = ay @ T @ ay, ax @ T @ ax
    if not (np.isfinite(num) and num > 0 and np.isfinite(den) and den > 0):
        return LLR_CLIP
    q = num / den
    if not (np.isfinite(q) and q > 0):
        return LLR_CLIP
    return min(LLR_CLIP, float(np.log(q)))


def cepstrum(a):
    P = len(a) - 1
    c = np.zeros(P + 1)
    for k in range(1, P + 1):
        s = 0.0
        for i in range(1, k):
            s += i * c[i] * a[k - i]
        c[k] = -(a[k] + s / k)
    return c[1:]


def cep_frame(cx, cy):
    return min(CEP_CLIP, 10 * np.sqrt(2) / np.log(10) * float(np.sqrt(np.sum((cx - cy) ** 2))))


# ---- critical bands ----------------------------------------------------------------------------------------------------------
def wss_products(pw):
    E = 10 * np.log10(np.maximum(pw, 1e-10))
    S = E[1:] - E[:-1]
    emax = np.max(E)
    W = np.empty(24)
    for b in range(24):
        if S[b] > 0:
            n = b
            while n <= 23 and S[n] > 0:
                n += 1
            pk = E[n]
        else:
            n = b
            while n >= 0 and S[n] <= 0:
                n -= 1
            pk = E[n + 1]
        W[b] = 20 / (20 + emax - E[b]) * (1 / (1 + pk - E[b]))
    return S, W


def wss_frame(X, Y, W):
    Sx, Wx = wss_products(W @ (np.abs(X) ** 2))
    Sy, Wy = wss_products(W @ (np.abs(Y) ** 2))
    Wb = 0.5 * (Wx + Wy)
    return float(np.sum(Wb * (Sx - Sy) ** 2) / np.sum(Wb))


def fwseg_frame(X, Y, W):
    ax, ay = np.abs(X), np.abs(Y)
    Bx, By = W @ (ax / np.sum(ax)), W @ (ay / np.sum(ay))
    num = den = 0.0
    for b in range(25):
        if Bx[b] == 0:
            continue
        w = Bx[b] ** 0.2
        num += w * 10 * np.log10(Bx[b] ** 2 / max((Bx[b] - By[b]) ** 2, EPS))
        den += w
    v = num / den if den > 0 else FW_LO
    return float(min(max(v, FW_LO), FW_HI))


# ---- the four measures -------------------------------------------------------------------------------------------------------
def frame_values(x, y, fs, lpc_order=None):
    """-> dict name -> array of M frame values."""
    x = np.asarray(x).astype(np.float64) + EPS
    y = np.asarray(y).astype(np.float64) + EPS
    assert x.shape == y.shape and x.ndim == 1
    P = default_order(fs) if lpc_order is None else int(lpc_order)
    N = nfft(fs)
    W = filters(fs)
    fx, fy = frames(x, fs), frames(y, fs)
    out = {m: np.empty(len(fx)) for m in NAMES}
    for j, (a, b) in enumerate(zip(fx, fy)):
        rx, ry = lags(a, P), lags(b, P)
        ax, ay = levinson(rx, P), levinson(ry, P)
        out["llr"][j] = llr_frame(rx, ax, ay)
        out["cep_dist"][j] = cep_frame(cepstrum(ax), cepstrum(ay))
        X, Y = np.fft.fft(a, N)[:N // 2], np.fft.fft(b, N)[:N // 2]
        out["wss"][j] = wss_frame(X, Y, W)
        out["fwseg_snr"][j] = fwseg_frame(X, Y, W)
    return out


def quality(x, y, fs, lpc_order=None):
    """{'llr', 'cep_dist', 'wss', 'fwseg_snr'}: trimmed means (95 %) of the first three, the plain mean of fwSNRseg; NaN for M = 0."""
    fv = frame_values(x, y, fs, lpc_order)
    if len(fv["llr"]) == 0:
        return {m: float("nan") for m in NAMES}
    return {"llr": trimmed_mean(fv["llr"]), "cep_dist": trimmed_mean(fv["cep_dist"]), "wss": trimmed_mean(fv["wss"]),
            "fwseg_snr": float(np.mean(fv["fwseg_snr"]))}
