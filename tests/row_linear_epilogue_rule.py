"""The gate and GIF epilogues of the row linear kernel (``include/aura_hip.h``, "Row linear: gate epilogue" and "Row
linear: GIF epilogue") restated in NumPy, as test infrastructure: the gate once in fp64 with its bound and once in fp32 as
the rule rounds it; the GIF step (the fp32 op sequence of ``oracle/aura_oracle.gif_run``), the T-mean (the rule of
``tests/test_host_neuron_rules.py``: one rounding of the fp32 quotient) and the mix in fp32.  Nothing here is measured on a
device.  ``e = 2^-24``; the dot product, its order and its bound ``d`` (bias and its rounding included) are those of
``tests/row_linear_rule.py``.

Every rounding of the epilogue is entered at a whole ulp, ``2e`` relatively, not at the half ulp that round-to-nearest
guarantees: the GPU test asks every element to stay within HALF its bound, and a single rounding may use its half ulp
in full, so a bound made of half ulps could not be met at half.  (``tests/row_linear_rule.py`` does the same for its last
rounding: ``2u |y|``.)

a         ``a = fl(t + u)``: the error of t and one rounding: ``da = d + 2e |a|``.
sigmoid   ``E = expf(-a)`` is within 1 ulp (the documented accuracy of the device function; the OpenCL limit is 3):
          relatively ``2e``.  ``p = fl(1 + E)`` and ``s = fl(1 / p)`` round once each (``2e`` each as above), and a
          relative error r of E moves ``1 / (1 + E)`` by at most ``r E / (1 + E) <= r`` relatively: ``s = sig(a) (1 + rho)``,
          ``|rho| <= 6e`` to first order; ``6.5 e`` holds the second-order terms.  Where E overflows (a < -88.7) s = 0
          against a sigmoid below 2^-127, and where E is subnormal (a > 87.3) its absolute error is far below e:
          ``2^-120`` covers both.  The sigmoid of the computed a against the sigmoid of the fp64 one: ``sig' = sig (1 -
          sig)`` changes by at most a factor ``exp(|delta|)`` over an interval of length delta, so
              g = s64 (1 - s64) da exp(da),      ds = g + 6.5 e (s64 + g) + 2^-120.
y         ``fl(s c)`` rounds once, ``fl(res + .)`` once: ``dy = |c| ds + 2e |s64 c| + 2e |y64|``, times ``1 + 2^-20`` for
          the second-order terms (the products of the above with one another)."""
import numpy as np

from tests import row_linear_rule as RULE

E24 = 2.0 ** -24


def sigmoid64(a):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(a >= 0, 1.0 / (1.0 + np.exp(-np.abs(a))), np.exp(-np.abs(a)) / (1.0 + np.exp(-np.abs(a))))


def gate64(x, W, b, u, c, res):
    """The rule in fp64 on the fp32 inputs: ``dict(y, bound, a, s)``.  ``W`` is the [N, K] block that is read."""
    lin = RULE.linear64(x, [W], [b])
    f64 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)
    u, c, res = f64(u), f64(c), f64(res)
    with np.errstate(over="ignore", invalid="ignore"):
        t, d = lin["y"][0], lin["bound"][0]
        a = t + u
        da = d + 2.0 * E24 * np.abs(a)
        s = sigmoid64(a)
        g = s * (1.0 - s) * da * np.exp(np.minimum(da, 700.0))
        ds = g + 6.5 * E24 * (s + g) + 2.0 ** -120
        y = res + s * c
        dy = (np.abs(c) * ds + 2.0 * E24 * np.abs(s * c) + 2.0 * E24 * np.abs(y)) * (1.0 + 2.0 ** -20)
    return dict(y=y, bound=dy, a=a, s=s)


def gate32(x, W, b, u, c, res):
    """The rule in fp32 (NumPy's exp in place of the device's expf: for known answers, not for bits)."""
    f32 = RULE._f32
    one = np.float32(1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        t = RULE.dot32(x, W)
        if b is not None:
            t = (t + f32(b)[None, :]).astype(np.float32)
        a = (t + f32(u)).astype(np.float32)
        s = (one / (one + np.exp(-a).astype(np.float32)).astype(np.float32)).astype(np.float32)
        return (f32(res) + (s * f32(c)).astype(np.float32)).astype(np.float32)


def hybrid_mix32(res, m, mean, gate):
    """The mix of the GIF epilogue's time-major form in fp32: ``g = fl(1 / fl(1 + exp(-gate)))`` and
    ``y = fl(res + fl(fl(fl(1 - g) m) + fl(g mean)))``: the HybridFFN's ``(1 - g) * mlp + g * snn`` and the layer's
    residual as torch evaluates ``res + ((1 - g) * m + g * mean)`` (NumPy's exp in place of the device's expf)."""
    f32 = RULE._f32
    one = np.float32(1.0)
    g = np.float32(one / np.float32(one + np.exp(np.float32(-gate)).astype(np.float32)))
    left = (np.float32(one - g) * f32(m)).astype(np.float32)
    right = (g * f32(mean)).astype(np.float32)
    return (f32(res) + (left + right).astype(np.float32)).astype(np.float32)


def gif_step32(v, theta, i_t, decay, L, alpha, threshold):
    """One fp32 GIF step, the op sequence of ``oracle/aura_oracle.gif_run`` (and ``csrc/aura_gif_model.inl``), every
    op rounded to fp32 on its own: returns ``(spike, v, theta)``."""
    f = np.float32
    v = f(f(f(v) * f(decay)) + f(i_t))
    cl = f(f(f(L) * f(theta)) * f(2.0))
    v = np.minimum(np.maximum(v, -cl), cl).astype(np.float32)
    nv = f(v / f(f(theta) + f(1e-6)))
    spike = np.minimum(np.maximum(np.floor(nv), f(0.0)), f(L)).astype(np.float32)
    v = f(v - f(spike * f(theta)))
    if alpha > 0.0:
        theta = f(f(f(theta) + f(f(alpha) * spike)) - f(f(alpha) * f(f(theta) - f(threshold))))
    return spike, v, theta


def gif_mean32(currents, T, decay, L, alpha, threshold):
    """The time-major form in fp32: ``currents`` [tokens * T, N] -> the mean over T [tokens, N], from fresh state."""
    c = RULE._f32(currents).reshape(-1, T, currents.shape[-1])
    v = np.zeros((c.shape[0], c.shape[2]), dtype=np.float32)
    theta = np.full_like(v, np.float32(threshold))
    acc = np.zeros_like(v)
    for t in range(T):
        spike, v, theta = gif_step32(v, theta, c[:, t], decay, L, alpha, threshold)
        acc = (acc + spike).astype(np.float32)
    return (acc / np.float32(T)).astype(np.float32)
