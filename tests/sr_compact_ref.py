"""The model of the compact super-resolution path (SRVGGNetCompact), written from DESIGN.md §6m alone, in torch on the CPU (no HIP, no project code), and the
exact integer convolutions the kernel tests compare with.

One set of half-rounded weights, two evaluations:
  M64  float64 throughout, nothing rounded in between
  Mh   float32 convolutions, every stored activation rounded to IEEE half exactly where §6m rounds: once per layer, after the whole epilogue
Both start from the same input tensor: the source's samples as halves in [0, 1] (tests/sr_ref.py input_tensor).  Weights are a dict in the state dict's names:
body.0 the first convolution, body.1 its PReLU slopes, body.2 k / body.2 k + 1 trunk layer k - 1, body.2 convs + 2 the last convolution."""
import numpy as np

# torch is imported where it is used, not when this module is (tests/sr_ref.py says why)


def keys(convs):
    """the state dict's keys in its own order, which is the flat order of hevc_amd/csrc/sr_compact_net.h"""
    out = []
    for i in range(convs + 1):
        out += [f"body.{2 * i}.weight", f"body.{2 * i}.bias", f"body.{2 * i + 1}.weight"]
    return out + [f"body.{2 * convs + 2}.weight", f"body.{2 * convs + 2}.bias"]


def shape(key, scale, convs):
    i = int(key.split(".")[1])
    if i % 2:
        return (64,)
    cout, cin = (3 * scale * scale if i == 2 * convs + 2 else 64), (3 if i == 0 else 64)
    return (cout, cin, 3, 3) if key.endswith(".weight") else (cout,)


def count(scale, convs):
    return sum(int(np.prod(shape(k, scale, convs))) for k in keys(convs))


def random_weights(scale, convs, seed, gain=1.0, tail_gain=1.0):
    """gaussian weights with Kaiming's variance (fan-in) times gain, the last convolution's times tail_gain; biases uniform within +-0.05; one slope per
    channel uniform in [-0.2, 0.6]; float32"""
    rng = np.random.default_rng(seed)
    out = {}
    last = 2 * convs + 2
    for k in keys(convs):
        s = shape(k, scale, convs)
        i = int(k.split(".")[1])
        if i % 2:
            out[k] = rng.uniform(-0.2, 0.6, s).astype(np.float32)
        elif k.endswith(".bias"):
            out[k] = rng.uniform(-0.05, 0.05, s).astype(np.float32)
        else:
            out[k] = (rng.standard_normal(s) * np.sqrt(2.0 / (s[1] * 9)) * (tail_gain if i == last else gain)).astype(np.float32)
    return out


def flatten(weights, convs):
    return np.concatenate([np.asarray(weights[k], np.float32).reshape(-1) for k in keys(convs)])


def half_round(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def pixel_shuffle(v, r):
    """[C r r, H, W] -> [C, r H, r W]: channel c r r + dy r + dx at (y, x) goes to channel c at (r y + dy, r x + dx)"""
    c = v.shape[0] // (r * r)
    h, w = v.shape[1:]
    return v.reshape(c, r, r, h, w).permute(0, 3, 1, 4, 2).reshape(c, h * r, w * r)


class Model:
    """mode "M64" or "Mh"; weights: key -> float32 array (convolution weights are rounded to half here; biases and slopes stay float32)"""

    def __init__(self, weights, scale, convs, mode):
        import torch
        self.scale, self.convs, self.half = scale, convs, mode == "Mh"
        self.dt = torch.float32 if self.half else torch.float64
        self.w = {k: torch.from_numpy(half_round(v) if np.ndim(v) == 4 else np.asarray(v, np.float32)).to(self.dt) for k, v in weights.items()}

    def store(self, v):
        return v.half().to(self.dt) if self.half else v

    def __call__(self, x_half):
        """x_half: [3, H, W] float16 array -> [3, scale H, scale W] array of the mode's float type"""
        import torch
        import torch.nn.functional as F
        with torch.no_grad():
            x = torch.from_numpy(np.asarray(x_half, np.float16).astype(np.float32)).to(self.dt)
            t = x
            for i in range(self.convs + 1):
                v = F.conv2d(t[None], self.w[f"body.{2 * i}.weight"], None, padding=1)[0] + self.w[f"body.{2 * i}.bias"][:, None, None]
                t = self.store(torch.where(v >= 0, v, v * self.w[f"body.{2 * i + 1}.weight"][:, None, None]))
            last = 2 * self.convs + 2
            r = self.scale
            v = F.conv2d(t[None], self.w[f"body.{last}.weight"], None, padding=1)[0] + self.w[f"body.{last}.bias"][:, None, None]
            v = v + x.repeat_interleave(r * r, dim=0)          # channel c r r + dy r + dx takes the source's component c: the nearest enlargement, before the shuffle
            return pixel_shuffle(self.store(v), r).numpy()


# ------------------------------------------------------------------------------------------------ the exact convolutions of the kernel tests
def _sums(x, w, bias):
    """the integer sums, worked out in float64 products of small integers (exact far below 2^53) and checked to be integers"""
    x = np.asarray(x, np.float64)
    h, wd, _ = x.shape
    xp = np.zeros((h + 2, wd + 2, x.shape[2]), np.float64)
    xp[1:-1, 1:-1] = x
    wi = np.asarray(w, np.float64)
    acc = np.zeros((h, wd, wi.shape[0]), np.float64)
    for ky in range(3):
        for kx in range(3):
            acc += xp[ky:ky + h, kx:kx + wd] @ wi[:, :, ky, kx].T
    acc += np.asarray(bias, np.float64)
    out = acc.astype(np.int64)
    assert np.array_equal(out, acc)
    return out


def conv_prelu_exact(x, w, bias, slopes):
    """x [H, W, Cin] and w [64, Cin, 3, 3] small integers, bias integers, slopes [64] dyadic fractions -> ([H, W, 64] float16, the integer sums).  Sums in
    int64, the PReLU in float64 on values that are exact in float32 (asserted), one rounding to half (numpy: nearest even)"""
    s = _sums(x, w, bias)
    v = s.astype(np.float64)
    v = np.where(v >= 0, v, v * np.asarray(slopes, np.float64))
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v), "a case whose result is not exact in float32"
    return v.astype(np.float32).astype(np.float16), s


def conv_tail_exact(x, w, bias, base, r):
    """x [H, W, 64] and w [3 r r, 64, 3, 3] small integers, bias integers, base [H, W, 3] multiples of 1 / 256 -> ([3, r H, r W] float16 planes, the same without
    the base).  v = sum + bias + base[c] for channel c r r + dy r + dx, exact in float32 (asserted), one rounding to half, stored at (r y + dy, r x + dx)"""
    s = _sums(x, w, bias).astype(np.float64)
    h, wd, _ = s.shape
    v = s + np.repeat(np.asarray(base, np.float64), r * r, axis=2)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v), "a case whose result is not exact in float32"

    def planes(a):
        return a.astype(np.float32).astype(np.float16).reshape(h, wd, 3, r, r).transpose(2, 0, 3, 1, 4).reshape(3, h * r, wd * r)
    return planes(v), planes(s)
