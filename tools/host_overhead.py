#!/usr/bin/env python3
"""Host-side cost of one decode-layer call (eager, no graph): where the microseconds go between Python and the kernel."""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "torch-bnb-fp4_amd")]
import torch  # noqa: E402
from torch import nn  # noqa: E402

import torch_bnb_fp4 as pkg  # noqa: E402

dev = torch.device("cuda", 0)
M = K = 4096
lin = nn.Linear(K, M).to(dev).to(torch.bfloat16)
fp4 = pkg.TorchFP4Linear(pkg.swap_linear_with_bnb_linear(lin).to(dev))
qd = fp4.quant_data
x = torch.randn(1, K, device=dev, dtype=torch.bfloat16)
fp4(x)


def bench(name, fn, n=3000):
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    print(f"{name:46s} host issue {t_issue / n * 1e6:6.2f} us/call   with GPU drain {t_all / n * 1e6:6.2f} us/call", flush=True)


with torch.inference_mode():
    bench("ext.gemv_fp4_bias (raw extension op)", lambda: pkg.ext.gemv_fp4_bias(x, qd._B_t, qd.absmax, qd.code, 64, qd.qtype, qd._shape_list, qd.bias))
    bench("QuantData.forward", lambda: qd.forward(x))
    bench("TorchFP4Linear.__call__", lambda: fp4(x))
    bench("functional gemm_4bit_inference (dtype lookup)", lambda: pkg.gemm_4bit_inference(x, qd._B_t, qd.absmax, qd.code, 64, torch.bfloat16, qd.quant_state.shape))
    bench("dense nn.Linear bf16 (hipBLASLt)", lambda: lin(x))
    bench("torch.add (one trivial torch op)", lambda: torch.add(x, x))
    xb = torch.randn(4, K, device=dev, dtype=torch.bfloat16)
    bench("TorchFP4Linear batch 4 (dequant + GEMM)", lambda: fp4(xb), n=1000)
    # the fused weight ops of the extension, whose operand checks share one preamble (csrc/torch_ext.cpp: weight_op)
    nf4_packed, nf4_absmax = pkg.ext.quantize_nf4(lin.weight.detach().contiguous(), 64)
    nf4_B = nf4_packed.t()
    bench("ext.gemv_nf4_fused (raw extension op)", lambda: pkg.ext.gemv_nf4_fused(x, nf4_B, nf4_absmax, 64, [M, K], None, None, 0))
    bench("ext.gemm_nf4_fused 4 rows (raw extension op)", lambda: pkg.ext.gemm_nf4_fused(xb, nf4_B, nf4_absmax, 64, [M, K], None, None, 0))
    bench("ext.gemm_small_fp4 4 rows (raw extension op)", lambda: pkg.ext.gemm_small_fp4(xb, qd._B_t, qd.absmax, 64, qd._shape_list, None))
