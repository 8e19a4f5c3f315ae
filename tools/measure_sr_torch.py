"""tools/measure_sr_torch.py — the yardstick beside tools/measure_sr.hip: the same RRDBNet (x4, 64 features, 32 growth channels) as a plain torch module in half
precision, channels-last, on the same device, timed with events: whole frames for 6 and 23 blocks at 480x270 and 960x540 (3 warm-up runs, 10 timed, median),
and the network's distinct convolution shapes alone (5 warm-up, 30 timed).  torch comes first in this process; the library is not loaded.  One JSON line per
measurement."""
import json
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F


class RDB(nn.Module):
    def __init__(self):
        super().__init__()
        self.c = nn.ModuleList([nn.Conv2d(64 + 32 * k, 64 if k == 4 else 32, 3, 1, 1) for k in range(5)])

    def forward(self, x):
        f = [x]
        for k in range(4):
            f.append(F.leaky_relu(self.c[k](torch.cat(f, 1)), 0.2))
        return self.c[4](torch.cat(f, 1)) * 0.2 + x


class RRDB(nn.Module):
    def __init__(self):
        super().__init__()
        self.r = nn.Sequential(RDB(), RDB(), RDB())

    def forward(self, x):
        return self.r(x) * 0.2 + x


class Net(nn.Module):
    def __init__(self, blocks):
        super().__init__()
        self.first = nn.Conv2d(3, 64, 3, 1, 1)
        self.body = nn.Sequential(*[RRDB() for _ in range(blocks)])
        self.cb, self.u1, self.u2, self.hr = (nn.Conv2d(64, 64, 3, 1, 1) for _ in range(4))
        self.last = nn.Conv2d(64, 3, 3, 1, 1)

    def forward(self, x):
        f = self.first(x)
        f = f + self.cb(self.body(f))
        f = F.leaky_relu(self.u1(F.interpolate(f, scale_factor=2, mode="nearest")), 0.2)
        f = F.leaky_relu(self.u2(F.interpolate(f, scale_factor=2, mode="nearest")), 0.2)
        return self.last(F.leaky_relu(self.hr(f), 0.2))


def timed(fn, warm, n):
    ts = []
    for i in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warm:
            ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    torch.backends.cudnn.benchmark = True
    dev = torch.device("cuda:0")
    with torch.no_grad():
        for sw, sh in ((480, 270), (960, 540)):
            for cin, cout, lvl in ((3, 64, 0), (64, 32, 0), (96, 32, 0), (128, 32, 0), (160, 32, 0), (192, 64, 0), (64, 64, 0), (64, 64, 1), (64, 64, 2), (64, 3, 2)):
                conv = nn.Conv2d(cin, cout, 3, 1, 1).to(dev).half().to(memory_format=torch.channels_last)
                x = torch.rand(1, cin, sh << lvl, sw << lvl, device=dev).half().to(memory_format=torch.channels_last)
                med, lo, hi = timed(lambda: conv(x), 5, 30)
                flop = 2.0 * 9 * cin * cout * (sw << lvl) * (sh << lvl)
                print(json.dumps({"case": f"torch conv {cin} -> {cout} at {sw << lvl}x{sh << lvl}", "median_us": round(med * 1000, 1), "min_us": round(lo * 1000, 1),
                                  "max_us": round(hi * 1000, 1), "tflops": round(flop / med * 1e-9, 1)}), flush=True)
            for blocks in (6, 23):
                net = Net(blocks).to(dev).half().to(memory_format=torch.channels_last).eval()
                x = torch.rand(1, 3, sh, sw, device=dev).half().to(memory_format=torch.channels_last)
                med, lo, hi = timed(lambda: net(x), 3, 10)
                print(json.dumps({"case": f"torch network x4 B={blocks} {sw}x{sh}", "median_ms": round(med, 2), "min_ms": round(lo, 2), "max_ms": round(hi, 2)}), flush=True)
                del net
                torch.cuda.empty_cache()


if __name__ == "__main__":
    sys.exit(main())
