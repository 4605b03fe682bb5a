"""Restatement of the MX fp8 operand format of precision="mxfp8" (include/theia_hip.h, theia_quantize_mx8) in torch, for the tests.

Blocks of 32 consecutive elements along K inside one row.  amax = max |x| over the block; amax == 0: scale byte 127 and 32 zero
bytes; otherwise e = clamp(floor(log2 amax) - 8, -127, 127), scale byte e + 127, element e4m3fn(RNE(clamp(x * 2^-e, -448, 448))).
Everything is exact in float64 (x * 2^-e is a power-of-two scaling of a bf16 / f32 value) up to the final e4m3 rounding, which is
torch's own float8_e4m3fn conversion (round to nearest even, subnormals included)."""
import torch


def quantize(x: torch.Tensor):
    """x [rows, K] bf16 / f32 (any strides) -> (uint8 e4m3 bytes [rows, K], uint8 E8M0 scales [rows, K/32]), on x's device"""
    rows, K = x.shape
    assert K % 32 == 0
    xb = x.double().reshape(rows, K // 32, 32)
    amax = xb.abs().amax(dim=-1)
    _, ex = torch.frexp(amax)  # amax = f * 2^ex, f in [0.5, 1)
    e = torch.where(amax == 0, torch.zeros_like(ex), (ex - 1 - 8).clamp(-127, 127))
    y = (xb * torch.pow(2.0, -e.double()).unsqueeze(-1)).clamp(-448.0, 448.0)
    q = y.float().to(torch.float8_e4m3fn).view(torch.uint8)
    q = torch.where((amax == 0).unsqueeze(-1), torch.zeros_like(q), q)
    return q.reshape(rows, K).contiguous(), (e + 127).to(torch.uint8)


def dequantize(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """(e4m3 bytes [rows, K], E8M0 scales [rows, K/32]) -> float64 [rows, K]"""
    rows, K = q.shape
    v = q.contiguous().view(torch.float8_e4m3fn).double().reshape(rows, K // 32, 32)
    return (v * torch.pow(2.0, s.double() - 127.0).unsqueeze(-1)).reshape(rows, K)
