"""The model of the learned super-resolution path, written from DESIGN.md §6l alone, in torch on the CPU (no HIP, no project code), and the exact integer
convolution the kernel tests compare with.

One set of half-rounded weights, two evaluations:
  M64  float64 throughout, nothing rounded in between
  Mh   float32 convolutions, every stored activation rounded to IEEE half exactly where §6l rounds: once per layer, after the whole epilogue
Both start from the same input tensor: the source's samples as halves in [0, 1] (input_tensor)."""
import numpy as np

SLOPE = 0.2
# torch is imported where it is used, not when this module is: in a pytest process the test files are collected before anything runs, and a torch that comes
# up at collection brings its own HIP runtime in front of the library's


def layer_names(blocks):
    """the layers in the flat order of the weights (hevc_amd/csrc/sr_net.h)"""
    return (["conv_first"] + [f"body.{i}.rdb{r}.conv{k}" for i in range(blocks) for r in (1, 2, 3) for k in (1, 2, 3, 4, 5)]
            + ["conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"])


def layer_shape(name, scale):
    """(cout, cin)"""
    if name == "conv_first":
        return 64, 12 if scale == 2 else 3
    if name == "conv_last":
        return 3, 64
    if ".conv" in name:
        k = int(name[-1])
        return (64 if k == 5 else 32), 64 + 32 * (k - 1)
    return 64, 64


def random_weights(scale, blocks, seed, gain=0.1):
    """gaussian weights with the variance of RRDBNet's initialisation (Kaiming, fan-in, times gain = 0.1), biases uniform within +-0.05; float32.  With 0.1 a
    layer passes on about a seventh of what it receives, so everything in front of conv_hr reaches the output below half precision; gain = 1 (plain Kaiming)
    keeps every layer's share of the output far above it: the cases that can see the trunk"""
    rng = np.random.default_rng(seed)
    out = {}
    for n in layer_names(blocks):
        cout, cin = layer_shape(n, scale)
        out[n + ".weight"] = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (cin * 9)) * gain).astype(np.float32)
        out[n + ".bias"] = rng.uniform(-0.05, 0.05, cout).astype(np.float32)
    return out


def flatten(weights, blocks):
    return np.concatenate([weights[n + s].reshape(-1) for n in layer_names(blocks) for s in (".weight", ".bias")]).astype(np.float32)


def half_round(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def input_tensor(planes, peak=None):
    """[3, H, W] R, G, B -> the halves the network reads, as float32.  Integers: float32(v) / float32(peak), a correctly rounded float32 division, then nearest
    even to half; floats: clamped to [0, 1], NaN 0, to half"""
    p = np.stack(planes)
    if peak is not None:
        x = np.minimum(p.astype(np.int64), peak).astype(np.float32) / np.float32(peak)
    else:
        x = p.astype(np.float32)
        x = np.where(x > 0, x, np.float32(0))
        x = np.where(x < 1, x, np.float32(1))
    return x.astype(np.float32).astype(np.float16)


def pixel_unshuffle(x):
    """[C, H, W] -> [4 C, H / 2, W / 2]: channel c 4 + dy 2 + dx at (y, x) is channel c at (2 y + dy, 2 x + dx)"""
    c, h, w = x.shape
    out = x.new_zeros((c * 4, h // 2, w // 2))
    for ch in range(c):
        for dy in range(2):
            for dx in range(2):
                out[ch * 4 + dy * 2 + dx] = x[ch, dy::2, dx::2]
    return out


def nearest2x(x):
    """[C, H, W] -> [C, 2 H, 2 W]: position (y, x) reads (y >> 1, x >> 1)"""
    import torch
    c, h, w = x.shape
    yy = torch.arange(2 * h) >> 1
    xx = torch.arange(2 * w) >> 1
    return x[:, yy][:, :, xx]


class Model:
    """mode "M64" or "Mh"; weights: name -> float32 array (rounded to half here)"""

    def __init__(self, weights, scale, blocks, mode):
        import torch
        self.scale, self.blocks, self.half = scale, blocks, mode == "Mh"
        self.dt = torch.float32 if self.half else torch.float64
        self.w = {k: torch.from_numpy(half_round(v) if k.endswith(".weight") else np.asarray(v, np.float32)).to(self.dt) for k, v in weights.items()}

    def conv(self, name, x, act=False, res=()):
        """one layer with its epilogue: v = acc + bias; LeakyReLU; v = v a + r for every (a, r) of res; one rounding to half"""
        import torch
        import torch.nn.functional as F
        v = F.conv2d(x[None], self.w[name + ".weight"], None, padding=1)[0] + self.w[name + ".bias"][:, None, None]
        if act:
            v = torch.where(v >= 0, v, v * torch.tensor(SLOPE, dtype=torch.float32).to(self.dt))
        for a, r in res:
            v = v * torch.tensor(a, dtype=torch.float32).to(self.dt) + r
        return v.half().to(self.dt) if self.half else v

    def rdb(self, p, x, outer=None):
        import torch
        x1 = self.conv(p + ".conv1", x, True)
        x2 = self.conv(p + ".conv2", torch.cat((x, x1)), True)
        x3 = self.conv(p + ".conv3", torch.cat((x, x1, x2)), True)
        x4 = self.conv(p + ".conv4", torch.cat((x, x1, x2, x3)), True)
        res = [(0.2, x)] + ([(0.2, outer)] if outer is not None else [])
        return self.conv(p + ".conv5", torch.cat((x, x1, x2, x3, x4)), False, res)

    def __call__(self, x_half):
        """x_half: [3, H, W] float16 array -> [3, scale H, scale W] array of the mode's float type"""
        import torch
        with torch.no_grad():
            x = torch.from_numpy(np.asarray(x_half, np.float16).astype(np.float32)).to(self.dt)
            if self.scale == 2:
                x = pixel_unshuffle(x)
            fea = self.conv("conv_first", x)
            t = fea
            for i in range(self.blocks):
                a = self.rdb(f"body.{i}.rdb1", t)
                b = self.rdb(f"body.{i}.rdb2", a)
                t = self.rdb(f"body.{i}.rdb3", b, outer=t)          # both residual pairs in one epilogue
            fea = self.conv("conv_body", t, False, [(1.0, fea)])
            fea = self.conv("conv_up1", nearest2x(fea), True)
            fea = self.conv("conv_up2", nearest2x(fea), True)
            return self.conv("conv_last", self.conv("conv_hr", fea, True)).numpy()


# ------------------------------------------------------------------------------------------------ the exact convolution of the kernel tests
def conv_exact(x, w, bias, up=False, act=False, slope=0.25, res=()):
    """x [H, W, Cin] and w [Cout, Cin, 3, 3] small integers (any numeric dtype), bias integers -> [H', W', Cout] float16.  Sums in int64 (exact), the epilogue in
    float64 on values that are exact dyadic fractions, one rounding to half (numpy: nearest even).  res: (a, r [H', W', Cout]) pairs"""
    x = np.asarray(x, np.int64)
    if up:
        x = x.repeat(2, axis=0).repeat(2, axis=1)
    h, wd, _ = x.shape
    xp = np.zeros((h + 2, wd + 2, x.shape[2]), np.int64)
    xp[1:-1, 1:-1] = x
    wi = np.asarray(w, np.int64)
    acc = np.zeros((h, wd, wi.shape[0]), np.int64)
    for ky in range(3):
        for kx in range(3):
            acc += xp[ky:ky + h, kx:kx + wd] @ wi[:, :, ky, kx].T
    v = (acc + np.asarray(bias, np.int64)).astype(np.float64)
    if act:
        v = np.where(v >= 0, v, v * slope)
    for a, r in res:
        v = v * a + np.asarray(r, np.float64)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v), "a case whose result is not exact in float32"
    return v.astype(np.float32).astype(np.float16)
