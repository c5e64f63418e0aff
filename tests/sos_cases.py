"""Coefficient tables and signals of the Biquad / SecondOrderSections tests.  The tables are literal numbers (designed once with scipy.signal: zpk
designs cut into sections with the gain kept apart), so no test needs scipy: rows of (b0, b1, b2, a1, a2) and the gain g."""
import numpy as np

SEED = 1776

TABLES = {
    'butter2_02': ([
        (1.0, 2.0, 1.0, -1.1429805025399011, 0.41280159809618877),
    ], 0.0674552738890719),
    'butter5_02': ([
        (1.0, 2.0, 1.0, -0.5095254494944288, 0.0),
        (1.0, 2.0, 1.0, -1.0965794655679617, 0.3554467621723905),
        (1.0, 1.0, 0.0, -1.3693171946832927, 0.6925691353878634),
    ], 0.001282581078960685),
    'butter8_02': ([
        (1.0, 2.0, 1.0, -1.0263514742610553, 0.26864019099379005),
        (1.0, 2.0, 1.0, -1.0868584613628944, 0.343430940165366),
        (1.0, 2.0, 1.0, -1.2197253651240232, 0.5076634651740437),
        (1.0, 2.0, 1.0, -1.4515795942478362, 0.794251053241888),
    ], 2.395964410377617e-05),
    'ellip6_001': ([
        (1.0, -1.9789961635621114, 0.9999999999999999, -1.9789841886394866, 0.9792003477303853),
        (1.0, -1.9967060475283307, 1.0, -1.9876417413314638, 0.988320501786239),
        (1.0, -1.9979662839346537, 0.9999999999999997, -1.9956683162942022, 0.9966721626448601),
    ], 0.0009882140089724676),
    'butter_bp4_030_031': ([
        (1.0, 2.0, 1.0, -1.1238931388492845, 0.971270171706141),
        (1.0, 2.0, 1.0, -1.14342426393917, 0.9715085523658537),
        (1.0, -2.0, 1.0, -1.1193673896857903, 0.9879298535593375),
        (1.0, -2.0, 1.0, -1.166715557022057, 0.9881721752229695),
    ], 5.8451424331444616e-08),
    'butter2_0001': ([
        (1.0, 2.0, 1.0, -1.995557124345789, 0.9955669720659747),
    ], 2.461930046414063e-06),
    'butter32_02': ([
        (1.0, 2.0, 1.0, -1.0195055091024368, 0.26017811268614255),
        (1.0, 2.0, 1.0, -1.0231504258132005, 0.2646834775129714),
        (1.0, 2.0, 1.0, -1.0304832737100313, 0.2737473759821206),
        (1.0, 2.0, 1.0, -1.0415908351397805, 0.2874770769735452),
        (1.0, 2.0, 1.0, -1.0566051685662186, 0.3060358137254701),
        (1.0, 2.0, 1.0, -1.0757058717854595, 0.329645581322501),
        (1.0, 2.0, 1.0, -1.0991230928174323, 0.358590858362157),
        (1.0, 2.0, 1.0, -1.1271412632836353, 0.39322322166356094),
        (1.0, 2.0, 1.0, -1.1601034944682453, 0.4339667800978025),
        (1.0, 2.0, 1.0, -1.198416515875155, 0.4813242789801474),
        (1.0, 2.0, 1.0, -1.2425559367534151, 0.5358836036731504),
        (1.0, 2.0, 1.0, -1.2930714537234438, 0.59832421656665),
        (1.0, 2.0, 1.0, -1.3505913852206857, 0.6694227619583721),
        (1.0, 2.0, 1.0, -1.4158255484085465, 0.7500566221138827),
        (1.0, 2.0, 1.0, -1.4895649562098696, 0.8412035427768962),
        (1.0, 2.0, 1.0, -1.5726760375921214, 0.9439344890488768),
    ], 3.4167008141246306e-19),
    'butter34_02': ([
        (1.0, 2.0, 1.0, -1.0194535873294586, 0.26011393384522885),
        (1.0, 2.0, 1.0, -1.0226813984125709, 0.264103727762483),
        (1.0, 2.0, 1.0, -1.029170752848076, 0.27212501097485714),
        (1.0, 2.0, 1.0, -1.0389896387804516, 0.28426182145058987),
        (1.0, 2.0, 1.0, -1.0522413484231867, 0.30064183538709993),
        (1.0, 2.0, 1.0, -1.069066051302575, 0.32143831184726007),
        (1.0, 2.0, 1.0, -1.0896428892444465, 0.34687268230541024),
        (1.0, 2.0, 1.0, -1.114192580509018, 0.37721776953505354),
        (1.0, 2.0, 1.0, -1.1429805025399011, 0.41280159809618877),
        (1.0, 2.0, 1.0, -1.1763201917641142, 0.4540117203260332),
        (1.0, 2.0, 1.0, -1.214577148431417, 0.5012999193790832),
        (1.0, 2.0, 1.0, -1.2581727556280073, 0.5551870533944481),
        (1.0, 2.0, 1.0, -1.3075880017295374, 0.616267656700821),
        (1.0, 2.0, 1.0, -1.3633665172784286, 0.6852136936032793),
        (1.0, 2.0, 1.0, -1.426116177200737, 0.7627765388322465),
        (1.0, 2.0, 1.0, -1.4965081471604302, 0.8497857987725506),
        (1.0, 2.0, 1.0, -1.5752717318007918, 0.9471429435395957),
    ], 2.3965367583301032e-20),
}
ZPK_BUTTER5 = (
    [(-1+0j), (-1+0j), (-1+0j), (-1+0j), (-1+0j)],
    [(0.6846585973416464+0.47308745541816344j), (0.5482897327839809+0.23414766942265602j), (0.5095254494944288+0j), (0.5482897327839809-0.23414766942265602j), (0.6846585973416464-0.47308745541816344j)],
    0.001282581078960685)
ZPK_ELLIP6 = (
    [(0.9894980817810557+0.14454600012318242j), (0.9983530237641653+0.057369329270508314j), (0.9989831419673268+0.04508527547977585j), (0.9894980817810557-0.14454600012318242j), (0.9983530237641653-0.057369329270508314j), (0.9989831419673268-0.04508527547977585j)],
    [(0.9894920943197433-0.010283141986456258j), (0.9938208706657319-0.02530965854067603j), (0.9978341581471011-0.03160942074328775j), (0.9894920943197433+0.010283141986456258j), (0.9938208706657319+0.02530965854067603j), (0.9978341581471011+0.03160942074328775j)],
    0.0009882140089724676)

INTEGRATOR = (1.0, 0.0, 0.0, -1.0, 0.0)            # y[i] = x[i] + y[i-1]: a pole ON the unit circle
FIR_ONLY = (1.0, 2.0, 3.0, 0.0, 0.0)               # a1 = a2 = 0: y = conv([1, 2, 3], x)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0)

# the tables of the accuracy comparison: every one of at most 16 sections (butter34_02 has 17 and is refused)
ACCURACY = ("butter2_02", "butter5_02", "butter8_02", "ellip6_001", "butter_bp4_030_031", "butter2_0001", "butter32_02")


def table(name):
    """(K x 5 Float64 array, gain)"""
    rows, g = TABLES[name]
    return np.array(rows, dtype=np.float64).reshape(len(rows), 5), g


def signal(n, ncols=1, dtype=np.float64, salt=0):
    """Standard normal samples, seed 1776 (+ salt), shape (n,) or (n, ncols), complex types with both parts drawn."""
    rng = np.random.default_rng(SEED + salt)
    dt = np.dtype(dtype)
    shape = (n,) if ncols == 1 else (n, ncols)
    x = rng.standard_normal(shape)
    if dt.kind == "c":
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dt)


def small_integers(n, ncols=1, dtype=np.float64, salt=0):
    rng = np.random.default_rng(SEED + 7 + salt)
    return rng.integers(-4, 5, size=(n,) if ncols == 1 else (n, ncols)).astype(dtype)


def emulate(tb, gain, x, dtype, segments=0, state=None, reverse=False, ld=None):
    """mdsp_sos_emulate_host on the columns of x ((n,) or (n, ncols), cast to the working type `dtype`): (y shaped like x, end state (2, K, ncols)).
    gain None: a Biquad (no gain).  state: (2, K, ncols) of dtype or None.  ld: leading dimension of both arrays (default n)."""
    import ctypes as C
    from dsp_jl_amd import _dev, _lib
    dt = np.dtype(dtype)
    tb = np.ascontiguousarray(tb, np.float64).reshape(-1, 5)
    K = len(tb)
    x = np.asarray(x)
    n = x.shape[0]
    cols = np.ascontiguousarray(x.reshape(n, -1).T.astype(dt))          # (ncols, n)
    ncols = cols.shape[0]
    ld = n if ld is None else ld
    xb, yb = np.zeros((ncols, max(ld, n)), dt), np.zeros((ncols, max(ld, n)), dt)     # (an ld below n is refused before anything is read)
    xb[:, :n] = cols
    st = None
    if state is not None:
        st = np.array(np.asarray(state, dt).reshape(2, K, ncols).transpose(2, 1, 0), dtype=dt, order="C", copy=True)     # element s + 2 (k + K c); a copy: the caller's array stays
    _lib.check(_lib.lib().mdsp_sos_emulate_host(xb.ctypes.data_as(C.c_void_p), ld, yb.ctypes.data_as(C.c_void_p), ld,
                                                None if st is None else st.ctypes.data_as(C.c_void_p), tb.ctypes.data_as(_lib.pdbl), K,
                                                1.0 if gain is None else float(gain), 0 if gain is None else 1, _dev.md_dtype(dt), n, ncols, int(segments),
                                                1 if reverse else 0))
    y = yb[:, :n].T.reshape(x.shape)
    return y, (None if st is None else st.transpose(2, 1, 0).copy())
