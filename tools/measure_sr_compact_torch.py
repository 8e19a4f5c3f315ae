"""tools/measure_sr_compact_torch.py — the yardstick beside tools/measure_sr_compact.hip: the same compact network (SRVGGNetCompact as DESIGN.md §6m defines
it: conv 3 -> 64, PReLU, `convs` times conv 64 -> 64 and PReLU with one slope per channel, conv 64 -> 48, pixel-shuffle 4, plus the source enlarged by nearest)
as a plain torch module in half precision, channels-last, on the same device, timed with events: whole frames for 16 and 32 convolutions at 480x270 and
960x540 (3 warm-up runs, 10 timed, median) and the 64 -> 64 convolution alone (5 warm-up, 30 timed).  Written from the definition; random weights, nothing is
downloaded.  torch comes first in this process; the library is not loaded.  One JSON line per measurement."""
import json
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F


class Compact(nn.Module):
    def __init__(self, convs, scale=4):
        super().__init__()
        layers = [nn.Conv2d(3, 64, 3, 1, 1), nn.PReLU(64)]
        for _ in range(convs):
            layers += [nn.Conv2d(64, 64, 3, 1, 1), nn.PReLU(64)]
        layers.append(nn.Conv2d(64, 3 * scale * scale, 3, 1, 1))
        self.body = nn.Sequential(*layers)
        self.scale = scale

    def forward(self, x):
        return F.pixel_shuffle(self.body(x), self.scale) + F.interpolate(x, scale_factor=self.scale, mode="nearest")


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
            conv = nn.Conv2d(64, 64, 3, 1, 1).to(dev).half().to(memory_format=torch.channels_last)
            x = torch.rand(1, 64, sh, sw, device=dev).half().to(memory_format=torch.channels_last)
            med, lo, hi = timed(lambda: conv(x), 5, 30)
            flop = 2.0 * 9 * 64 * 64 * sw * sh
            print(json.dumps({"case": f"torch conv 64 -> 64 at {sw}x{sh}", "median_us": round(med * 1000, 1), "min_us": round(lo * 1000, 1),
                              "max_us": round(hi * 1000, 1), "tflops": round(flop / med * 1e-9, 1)}), flush=True)
            for convs in (16, 32):
                net = Compact(convs).to(dev).half().to(memory_format=torch.channels_last).eval()
                x = torch.rand(1, 3, sh, sw, device=dev).half().to(memory_format=torch.channels_last)
                med, lo, hi = timed(lambda: net(x), 3, 10)
                flop = 2.0 * 9 * (3 * 64 + convs * 64 * 64 + 64 * 48) * sw * sh
                print(json.dumps({"case": f"torch compact network x4 convs={convs} {sw}x{sh}", "median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                                  "tflops": round(flop / med * 1e-9, 1)}), flush=True)
                del net
                torch.cuda.empty_cache()


if __name__ == "__main__":
    sys.exit(main())
