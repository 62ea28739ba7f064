"""Split-K factor sweep on the layers whose 128x128-tile grid leaves CUs idle at B = 64: dir_conv2d_splitk_forward through
functional.conv2d_nhwc(splits=S, workspace=...) against the best tiled variant of the engine's ConvOp."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dir_amd import _capi, engine as E, functional as F  # noqa: E402

LAYERS = [  # H, Cin, Cout, k, stride, pre
    (8, 512, 512, 3, 1, False), (16, 512, 512, 3, 2, False), (8, 2048, 512, 1, 1, False), (16, 1024, 512, 1, 1, False),
    (16, 128, 128, 3, 1, False), (16, 1024, 128, 1, 1, True), (16, 2304, 128, 1, 1, True), (16, 512, 128, 1, 1, True),
    (16, 256, 256, 3, 1, False), (16, 1024, 256, 1, 1, False), (8, 512, 2048, 1, 1, False), (8, 2048, 2048, 3, 1, False),
]
B = 64


def timeit(fn, n=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


for H, Cin, Cout, k, stride, pre in LAYERS:
    w = torch.randn(Cout, Cin, k, k) * (Cin * k * k) ** -0.5
    prep = (torch.rand(Cin).cuda() + 0.5, torch.randn(Cin).cuda()) if pre else None
    scale, shift = torch.ones(Cout).cuda(), torch.zeros(Cout).cuda()
    op = E.ConvOp(w.cuda(), torch.bfloat16, stride=stride, pad=k // 2, scale=scale, shift=shift, relu=True, pre=prep, pre_relu=pre)
    x = torch.randn(B, H, H, Cin, device='cuda').to(torch.bfloat16)
    best = None
    for v in E.DirEngine.CONV_VARIANTS:
        E._TLS.variant = v
        t = timeit(lambda: op(x))
        if best is None or t < best[0]:
            best = (t, v)
    E._TLS.variant = None
    nk = k * k * Cin // 64
    Ho = (H + 2 * (k // 2) - k) // stride + 1
    out = torch.empty(B, Ho, Ho, Cout, device='cuda', dtype=torch.bfloat16)
    d = _capi.ConvDesc(B, H, H, Cin, Cin, 0, Cout, Cout, 0, 0, 0, k, k, stride, k // 2, _capi.DT_BF16, _capi.DT_BF16, 0, 0, 0, 0.0)
    line = ''
    for S in (2, 3, 4, 6, 8, 12, 16):
        if S > nk:
            continue
        # the split launch itself: workspace made once (the kernel leaves its arrival counters zero), output buffer re-used
        ws = torch.zeros(_capi.lib().dir_conv2d_splitk_workspace_bytes(d, S), dtype=torch.uint8, device='cuda')
        line += '  S=%d %5.1f' % (S, timeit(lambda: F.conv2d_nhwc(x, op.w, stride=stride, pad=k // 2, scale=scale, shift=shift, relu=True,
                                                                    pre_scale=prep[0] if pre else None, pre_shift=prep[1] if pre else None, pre_relu=pre,
                                                                    out=out, splits=S, workspace=ws)))
    gf = 2.0 * B * Ho * Ho * Cout * k * k * Cin / 1e9
    print('M=%5d N=%4d K=%5d %s: best tiled %5.1f us (variant %2d, %4.0f TF) |%s' % (B * Ho * Ho, Cout, k * k * Cin, 'pre' if pre else '   ', best[0], best[1],
                                                                                    gf / best[0] / 1e3, line))
