"""BN254 optimal ate pairing, restated literally on Python integers.

The definition the device and host deciders are checked against:
  Fp2  = Fp[u] / (u^2 + 1)
  Fp6  = Fp2[v] / (v^3 - xi),  xi = 9 + u
  Fp12 = Fp6[w] / (w^2 - v)
  E'   : y^2 = x^3 + 3 / xi over Fp2 (D-type twist), (x', y') -> (x' w^2, y' w^3)
  e(P, Q) = (f_{6x+2,Q}(P) l_{T,pi Q}(P) l_{T + pi Q, -pi^2 Q}(P)) ^ ((p^12 - 1) / r)
Affine G2 steps, full Fp12 products and a plain square-and-multiply by
(p^12 - 1) // r: nothing here is an optimisation.  An Fp2 value is a pair, an
Fp6 value a triple of pairs, an Fp12 value a pair of triples.
"""
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
X = 4965661367192848881
LOOP = 6 * X + 2
assert P == 36 * X**4 + 36 * X**3 + 24 * X**2 + 6 * X + 1
assert R == 36 * X**4 + 36 * X**3 + 18 * X**2 + 6 * X + 1
assert LOOP == 29793968203157093288
FINAL_EXP = (P**12 - 1) // R
assert (P**12 - 1) % R == 0

G1 = (1, 2)
G2 = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
       11559732032986387107991004021392285783925812861821192530917403151452391805634),
      (8495653923123431417604973247489272438418190587263600148770280649306958101930,
       4082367875863433681332203403145435568316851327593401208105741076214120093531))

# ---------------------------------------------------------------- Fp2
F2_ZERO, F2_ONE = (0, 0), (1, 0)
XI = (9, 1)


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_scale(a, k):
    return (a[0] * k % P, a[1] * k % P)


def f2_conj(a):
    return (a[0], -a[1] % P)


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], P - 2, P)
    return (a[0] * n % P, -a[1] * n % P)


def f2_pow(a, e):
    r = F2_ONE
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_mul(a, a)
        e >>= 1
    return r


B2 = f2_mul((3, 0), f2_inv(XI))  # 3 / xi

# ---------------------------------------------------------------- Fp6
F6_ZERO = (F2_ZERO, F2_ZERO, F2_ZERO)
F6_ONE = (F2_ONE, F2_ZERO, F2_ZERO)


def f6_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def f6_sub(a, b):
    return tuple(f2_sub(x, y) for x, y in zip(a, b))


def f6_mul(a, b):
    # schoolbook in v, v^3 = xi
    c = [F2_ZERO] * 5
    for i in range(3):
        for j in range(3):
            c[i + j] = f2_add(c[i + j], f2_mul(a[i], b[j]))
    return (f2_add(c[0], f2_mul(XI, c[3])), f2_add(c[1], f2_mul(XI, c[4])), c[2])


def f6_mul_v(a):
    return (f2_mul(XI, a[2]), a[0], a[1])


# ---------------------------------------------------------------- Fp12
F12_ONE = (F6_ONE, F6_ZERO)


def f12_mul(a, b):
    # (a0 + a1 w)(b0 + b1 w), w^2 = v
    return (f6_add(f6_mul(a[0], b[0]), f6_mul_v(f6_mul(a[1], b[1]))),
            f6_add(f6_mul(a[0], b[1]), f6_mul(a[1], b[0])))


def f12_pow(a, e):
    r = F12_ONE
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def f12_flat(a):
    """The 12 Fp coefficients in the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1."""
    return [c for half in a for f2 in half for c in f2]


# ---------------------------------------------------------------- G1 (affine, None = identity)
def g1_on_curve(Pt):
    return Pt is None or (Pt[1] * Pt[1] - Pt[0] ** 3 - 3) % P == 0


def g1_neg(Pt):
    return None if Pt is None else (Pt[0], -Pt[1] % P)


def g1_add(A, Bp):
    if A is None:
        return Bp
    if Bp is None:
        return A
    if A[0] == Bp[0]:
        if (A[1] + Bp[1]) % P == 0:
            return None
        lam = 3 * A[0] * A[0] * pow(2 * A[1], P - 2, P) % P
    else:
        lam = (Bp[1] - A[1]) * pow(Bp[0] - A[0], P - 2, P) % P
    x = (lam * lam - A[0] - Bp[0]) % P
    return (x, (lam * (A[0] - x) - A[1]) % P)


def g1_mul(k, Pt):
    k %= R
    acc = None
    while k:
        if k & 1:
            acc = g1_add(acc, Pt)
        Pt = g1_add(Pt, Pt)
        k >>= 1
    return acc


# ---------------------------------------------------------------- G2 on the twist (affine over Fp2)
def g2_on_curve(Q):
    if Q is None:
        return True
    x, y = Q
    return f2_sub(f2_mul(y, y), f2_add(f2_mul(x, f2_mul(x, x)), B2)) == F2_ZERO


def g2_neg(Q):
    return None if Q is None else (Q[0], f2_neg(Q[1]))


def g2_slope(T, Q):
    """Slope of the line through T and Q (the tangent when T == Q); None for a vertical line."""
    if T[0] == Q[0]:
        if f2_add(T[1], Q[1]) == F2_ZERO:
            return None
        return f2_mul(f2_scale(f2_mul(T[0], T[0]), 3), f2_inv(f2_scale(T[1], 2)))
    return f2_mul(f2_sub(Q[1], T[1]), f2_inv(f2_sub(Q[0], T[0])))


def g2_add(T, Q):
    if T is None:
        return Q
    if Q is None:
        return T
    lam = g2_slope(T, Q)
    if lam is None:
        return None
    x = f2_sub(f2_sub(f2_mul(lam, lam), T[0]), Q[0])
    return (x, f2_sub(f2_mul(lam, f2_sub(T[0], x)), T[1]))


def g2_mul(k, Q, reduce=True):
    """[k]Q; reduce=False keeps k as given (the order check multiplies by r itself)."""
    if reduce:
        k %= R
    acc = None
    while k:
        if k & 1:
            acc = g2_add(acc, Q)
        Q = g2_add(Q, Q)
        k >>= 1
    return acc


FROB_X = f2_pow(XI, (P - 1) // 3)
FROB_Y = f2_pow(XI, (P - 1) // 2)


def g2_frobenius(Q):
    """pi(x', y') = (conj(x') xi^((p-1)/3), conj(y') xi^((p-1)/2))"""
    return (f2_mul(f2_conj(Q[0]), FROB_X), f2_mul(f2_conj(Q[1]), FROB_Y))


# ---------------------------------------------------------------- the pairing
def line(T, lam, Pt):
    """y_P - (lam x_P) w + (lam x_T - y_T) w^3, with w^3 = v w."""
    c = f2_sub(f2_mul(lam, T[0]), T[1])
    return (((Pt[1] % P, 0), F2_ZERO, F2_ZERO), (f2_neg(f2_scale(lam, Pt[0])), c, F2_ZERO))


def miller(Pt, Q):
    """f_{6x+2,Q}(P) l_{T,pi Q}(P) l_{T+pi Q,-pi^2 Q}(P); 1 when either point is the identity."""
    if Pt is None or Q is None:
        return F12_ONE
    f, T = F12_ONE, Q
    for bit in bin(LOOP)[3:]:
        f = f12_mul(f, f)
        lam = g2_slope(T, T)
        f = f12_mul(f, line(T, lam, Pt))
        T = g2_add(T, T)
        if bit == "1":
            lam = g2_slope(T, Q)
            f = f12_mul(f, line(T, lam, Pt))
            T = g2_add(T, Q)
    q1 = g2_frobenius(Q)
    q2 = g2_neg(g2_frobenius(q1))
    lam = g2_slope(T, q1)
    f = f12_mul(f, line(T, lam, Pt))
    T = g2_add(T, q1)
    lam = g2_slope(T, q2)
    f = f12_mul(f, line(T, lam, Pt))
    return f


def final_exp(f):
    return f12_pow(f, FINAL_EXP)


def pairing(Pt, Q):
    return final_exp(miller(Pt, Q))


def decide_gt(A, C, s_g2, g2=G2):
    """e(A, s_g2) e(C, g2): the value whose equality with 1 the decider reports."""
    return final_exp(f12_mul(miller(A, s_g2), miller(C, g2)))


def accum_gt(w, zw, f, e, s_g2, g2=G2):
    """The decider's value for an accumulator quad: A = w, C = -(zw + f + e)."""
    return decide_gt(w, g1_neg(g1_add(g1_add(zw, f), e)), s_g2, g2)


def honest_W(F, e, z, tau):
    """Discrete log of the KZG witness of a rotation set: (F - e) / (tau - z) mod r, F the set's
    commitment discrete log and e its evaluation at z."""
    return (F - e) * pow((tau - z) % R, R - 2, R) % R


# ---------------------------------------------------------------- the ABI's words
R256 = 1 << 256


def fp_words(v):
    """Montgomery (R = 2^256) 4 x u64 little endian"""
    v = v * R256 % P
    return [(v >> (64 * i)) & (2**64 - 1) for i in range(4)]


def words_fp(ws):
    v = sum(int(x) << (64 * i) for i, x in enumerate(ws))
    return v * pow(R256, P - 2, P) % P


def g1_words(Pt):
    return [0] * 8 if Pt is None else fp_words(Pt[0]) + fp_words(Pt[1])


def g2_words(Q):
    """16 x u64: x.c0, x.c1, y.c0, y.c1 (the identity, which pm_pairing_create refuses, as zeros)"""
    if Q is None:
        return [0] * 16
    return fp_words(Q[0][0]) + fp_words(Q[0][1]) + fp_words(Q[1][0]) + fp_words(Q[1][1])


def gt_words(f):
    return [w for c in f12_flat(f) for w in fp_words(c)]
