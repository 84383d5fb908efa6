"""The optimizers' references for the tests (test infrastructure, not collected: no `test_` prefix).

`scalars64` / `step64`: a float64 NumPy restatement of the reference's RectifiedAdam and AdamW (engine/optimizers.py), the
step's scalars included -- what the fp64 bars compare with.  `element32`: the element formula in float32 NumPy, one rounding
per operation in the order include/masklab_hip.h states, taking the step's scalars AS GIVEN (the device's own struct read
back) -- what the element bits compare with.  `magnitudes`: S, the uncancelled magnitude of each result.  `case`: the inputs."""
import numpy as np

KINDS = ("RectifiedAdam", "AdamW")
DEFAULTS = {"RectifiedAdam": dict(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, decay=0., weight_decay=0.),
            "AdamW": dict(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=0., weight_decay=1e-4)}
TINY = float(np.finfo(np.float32).tiny)


def hyper(kind, **over):
    """The reference's defaults of `kind` with `over` on top; init_lr = the constructor's lr, as the reference keeps it."""
    h = {**DEFAULTS[kind], **over}
    h.setdefault("init_lr", h["lr"])
    return h


def scalars64(kind, iterations, lr, h):
    """The scalars of the step that starts with `iterations` steps taken and learning rate `lr`, float64."""
    it = float(iterations)
    t = it + 1.
    if h["decay"] > 0:
        lr = lr / (1. + h["decay"] * it)
    b1t, b2t = h["beta_1"] ** t, h["beta_2"] ** t
    s = dict(beta_1=h["beta_1"], one_minus_beta_1=1. - h["beta_1"], beta_2=h["beta_2"], one_minus_beta_2=1. - h["beta_2"],
             epsilon=h["epsilon"], lr=lr, step=0., wd_lr=0., lr_t=0., eta_wd=0., rectified=1, decays=int(h["weight_decay"] != 0))
    if kind == "RectifiedAdam":
        n_max = 2. / (1. - h["beta_2"]) - 1.
        n = n_max - 2. * t * b2t / (1. - b2t)
        s["n_sma"] = n
        s["rectified"] = int(n > 5.)
        if s["rectified"]:
            s["step"] = lr * np.sqrt((1. - b2t) * (n - 4.) / (n_max - 4.) * (n - 2.) / n * n_max / (n_max - 2.)) / (1. - b1t)
        else:
            s["step"] = lr / (1. - b1t)
        s["wd_lr"] = h["weight_decay"] * lr
    else:
        s["lr_t"] = lr * np.sqrt(1. - b2t) / (1. - b1t)
        s["eta_wd"] = lr / h["init_lr"] * h["weight_decay"]
    return s


def _element(kind, s, p, g, m, v):
    """The element formula in the dtype of its inputs (every scalar of `s` already in that dtype).
    -> (p', m', v', decay term, update term)"""
    m1 = s["beta_1"] * m + s["one_minus_beta_1"] * g
    v1 = s["beta_2"] * v + s["one_minus_beta_2"] * (g * g)
    if kind == "RectifiedAdam":
        dec = s["wd_lr"] * p if s["decays"] else np.zeros_like(p)
        p_ = p - dec if s["decays"] else p
        upd = s["step"] * (m1 / (np.sqrt(v1) + s["epsilon"])) if s["rectified"] else s["step"] * m1
        return p_ - upd, m1, v1, dec, upd
    upd = s["lr_t"] * m1 / (np.sqrt(v1) + s["epsilon"])
    dec = s["eta_wd"] * p
    return p - upd - dec, m1, v1, dec, upd


def step64(kind, s64, p, g, m, v):
    """One step in float64 from the given state (any float dtype) with the float64 scalars `s64`. -> (p', m', v')"""
    return _element(kind, s64, *(np.asarray(a, dtype=np.float64) for a in (p, g, m, v)))[:3]


FLOAT_FIELDS = ("beta_1", "one_minus_beta_1", "beta_2", "one_minus_beta_2", "epsilon", "lr", "step", "wd_lr", "lr_t", "eta_wd")


def as_f32(s):
    """Scalars (a dict, or the device's struct read back) -> dict of np.float32 values and the two flags."""
    get = (lambda k: s[k]) if isinstance(s, dict) else (lambda k: getattr(s, k))
    out = {k: np.float32(get(k)) for k in FLOAT_FIELDS}
    out["rectified"], out["decays"] = int(get("rectified")), int(get("decays"))
    return out


def element32(kind, s, p, g, m, v):
    """One step in float32 NumPy with the scalars as given. -> (p', m', v'), float32"""
    assert all(a.dtype == np.float32 for a in (p, g, m, v))
    out = _element(kind, as_f32(s), p, g, m, v)[:3]
    assert all(a.dtype == np.float32 for a in out)
    return out


def intermediates32(kind, s, p, g, m, v):
    """Every float32 intermediate of element32, for the no-subnormal assertion."""
    s = as_f32(s)
    m1 = s["beta_1"] * m + s["one_minus_beta_1"] * g
    v1 = s["beta_2"] * v + s["one_minus_beta_2"] * (g * g)
    den = np.sqrt(v1) + s["epsilon"]
    vals = [s["beta_1"] * m, s["one_minus_beta_1"] * g, m1, g * g, s["one_minus_beta_2"] * (g * g), s["beta_2"] * v, v1,
            np.sqrt(v1), den, *_element(kind, s, p, g, m, v)]
    vals += [m1 / den] if kind == "RectifiedAdam" else [s["lr_t"] * m1]
    return vals


def no_subnormals(arrays):
    """True if no value of the arrays is a nonzero float32 below the smallest normal."""
    return all(not np.any((a != 0) & (np.abs(a) < TINY)) for a in arrays)


def magnitudes(kind, s64, p, g, m, v):
    """S = (S_p, S_m, S_v): what each result's terms add up to without cancellation, float64."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    _, _, v1, dec, upd = _element(kind, s64, p, g, m, v)
    return np.abs(p) + np.abs(dec) + np.abs(upd), s64["beta_1"] * np.abs(m) + s64["one_minus_beta_1"] * np.abs(g), v1


def case(sizes, seed):
    """p ~ N(0, 1) per tensor of `sizes`. -> list of float32 arrays"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(np.float32) for n in sizes]


def gradients(sizes, seed, step):
    """g = N(0, 1) * 10^U(-3, 1) per element, fresh for every (seed, step) and independent of p. -> list of float32 arrays"""
    rng = np.random.default_rng([seed, 1000 + step])
    return [(rng.standard_normal(n) * 10. ** rng.uniform(-3, 1, n)).astype(np.float32) for n in sizes]


class Trajectory:
    """A float64 run of one optimizer over a list of tensors from zero moments: the restatement, driven like the product."""

    def __init__(self, kind, params, **over):
        self.kind, self.h = kind, hyper(kind, **over)
        self.lr, self.iterations = self.h["lr"], 0
        self.p = [np.asarray(a, dtype=np.float64).copy() for a in params]
        self.m = [np.zeros_like(a) for a in self.p]
        self.v = [np.zeros_like(a) for a in self.p]

    def step(self, grads):
        s = scalars64(self.kind, self.iterations, self.lr, self.h)
        for i, g in enumerate(grads):
            self.p[i], self.m[i], self.v[i] = step64(self.kind, s, self.p[i], g, self.m[i], self.v[i])
        self.iterations += 1
        return s
