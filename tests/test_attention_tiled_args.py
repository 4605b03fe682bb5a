"""Argument checks of the key-tiled attention path (n > 256), without a GPU: every case below fails a check (the cap, or an output
overlapping an input) before anything is launched."""


def test_tiled_attention_cap_and_overlap_errors():
    from theia_amd import _native as N
    lib = N.lib()
    # beyond the cap
    assert lib.theia_attention_fwd(4096, 1 << 40, 1 << 41, 1, 8193, 3, N.BF16, None) == -1
    assert b"n=8193 must be in [1,8192]" in lib.theia_last_error()
    assert lib.theia_attention_bwd(4096, 1 << 40, 1 << 41, 1 << 42, 1 << 43, 1 << 44, 2, 9000, 12, N.F32, None) == -1
    assert b"n=9000" in lib.theia_last_error()
    # n = 300 is in range now; outputs overlapping the input are refused
    assert lib.theia_attention_fwd(4096, 4096, 1 << 40, 1, 300, 3, N.F32, None) == -1 and b"overlap" in lib.theia_last_error()
    assert lib.theia_attention_fwd(1 << 40, 4096, 4096 + 64, 1, 300, 3, N.BF16, None) == -1 and b"overlap" in lib.theia_last_error()
    assert lib.theia_attention_bwd(4096, 1 << 40, 1 << 41, 1 << 42, 4096, 1 << 44, 1, 257, 3, N.BF16, None) == -1
    assert b"overlap" in lib.theia_last_error()
    assert lib.theia_attention_bwd(4096, 1 << 40, 1 << 41, 1 << 42, 1 << 43, 1 << 41, 1, 257, 3, N.F32, None) == -1
    assert b"overlap" in lib.theia_last_error()
    assert lib.theia_attention_fwd(4096, 1 << 40, 1 << 41, 1, 0, 3, N.F32, None) == -1 and b"positive" in lib.theia_last_error()


def test_token_cap_of_the_backbone():
    from theia_amd.models.backbones import MAX_TOKENS
    assert MAX_TOKENS == 8192

