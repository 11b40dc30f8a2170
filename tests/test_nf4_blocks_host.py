"""fp4_hip_gemm_blocks_nf4's argument check (csrc/gemm_blocks_nf4.hip) through the C ABI, and the routing predicate beside it, without a GPU:
every call below is refused, or found empty, before any HIP call."""
import ctypes

import pytest
import torch

import hipabi

OK, INVALID, UNSUPPORTED, GATED = hipabi.OK, hipabi.ERR_INVALID, hipabi.ERR_UNSUPPORTED, hipabi.EPILOGUE_SILU_MUL_PAIRS
D = 0x1000  # a 16-byte aligned non-null "pointer": nothing below dereferences it


def call(x=D, packed=D, absmax=D, out=D, B=4, M=64, K=512, blocksize=128, dtype=hipabi.BF16, epilogue=hipabi.EPILOGUE_NONE):
    f = hipabi.lib().fp4_hip_gemm_blocks_nf4
    f.argtypes, f.restype = [ctypes.c_void_p] * 6 + [ctypes.c_int64] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p], ctypes.c_int
    return f(x, packed, absmax, None, None, out, B, M, K, blocksize, dtype, epilogue, None)


REFUSALS = [(dict(B=-1), INVALID), (dict(M=-1), INVALID), (dict(K=0), INVALID), (dict(blocksize=0), INVALID), (dict(epilogue=7), INVALID),
            (dict(M=63, epilogue=GATED), INVALID), (dict(x=None), INVALID), (dict(absmax=None), INVALID), (dict(out=None), INVALID),
            (dict(B=65), UNSUPPORTED), (dict(blocksize=64), UNSUPPORTED), (dict(blocksize=96, K=960), UNSUPPORTED),
            (dict(blocksize=8192, K=8192), UNSUPPORTED), (dict(K=192), UNSUPPORTED), (dict(dtype=hipabi.F32), UNSUPPORTED),
            (dict(x=D + 2), UNSUPPORTED), (dict(packed=D + 8), UNSUPPORTED), (dict(M=2**30 + 1), UNSUPPORTED),
            (dict(K=2**25, blocksize=4096), UNSUPPORTED)]


@pytest.mark.parametrize("kw,status", REFUSALS, ids=[str(r[0]) for r in REFUSALS])
def test_every_refusal_has_its_status_and_names_the_entry_point(kw, status):
    assert call(**kw) == status
    msg = hipabi.last_error()
    assert msg.startswith("fp4_hip_gemm_blocks_nf4:") and (status == INVALID or "not covered" in msg), msg  # "not covered": what the op's callers catch
    assert kw.get("blocksize") != 64 or "fp4_hip_gemm_fused_nf4" in msg  # the kernel that owns that block size


def test_an_empty_problem_is_ok_whatever_the_pointers_are():
    nulls = dict(x=None, packed=None, absmax=None, out=None)
    assert all(call(epilogue=e, **nulls, **empty) == OK for e in (hipabi.EPILOGUE_NONE, GATED) for empty in (dict(M=0), dict(B=0)))
    for bs in (128, 256, 512, 1024, 2048, 4096):  # every covered block size gets as far as the pointer check
        assert call(K=4096, blocksize=bs, B=0, **nulls) == OK and call(K=4096, blocksize=bs, out=None) == INVALID


def test_the_routing_predicate():
    from torch_bnb_fp4.quant_data import nf4_batched_covers, nf4_blocks_covers as covers

    for dtype in (torch.float16, torch.bfloat16):
        for bs in (128, 256, 512, 1024, 2048, 4096):
            assert all(covers(rows, 4096, bs, dtype) for rows in (2, 16, 17, 64)) and not nf4_batched_covers(8, 4096, bs, dtype)
            assert not any(covers(rows, 4096, bs, dtype) for rows in (0, 1, 65, 128))  # one row is the GEMV's
        assert covers(8, 384, 128, dtype) and not covers(8, 192, 128, dtype)  # K = 128 * odd; K % blocksize != 0
        assert not any(covers(8, 8192, bs, dtype) for bs in (32, 64, 96, 192, 8192))
    assert not covers(8, 4096, 128, torch.float32)
    # the two cells profiles/nf4_blocks.json does not show ahead are closed from 33 rows on, and nothing around them
    for K, bs in ((14336, 128), (11008, 256)):
        assert not covers(64, K, bs, torch.bfloat16) and not covers(33, K, bs, torch.bfloat16)
        assert covers(32, K, bs, torch.bfloat16) and covers(64, K, bs, torch.float16)
    assert covers(64, 14336, 256, torch.bfloat16) and covers(64, 11008, 128, torch.bfloat16)
