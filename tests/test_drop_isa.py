"""The reduced-quality decoders' compiled gfx950 code (hipcc cross-compiles here; no GPU needed): bpc_decode_drop_kernel
meets the two limits the guard of tests/test_isa_guards.py sets for the k = 0 decoder's existing forms -- a plane loop free
of scratch traffic (at most 80 scratch instructions after the first v_bcnt_u32_b32, all of them the epilogue's) and a private
segment of at most 192 bytes -- so it runs eight waves a SIMD in 64 registers as they do."""
import re

import pytest

from test_isa_guards import _kernel_body, device_asm  # noqa: F401  (the fixture: one compile of the library's device code)

DROP_KERNELS = ("22bpc_decode_drop_kernelILb0ELb0E", "22bpc_decode_drop_kernelILb1ELb0E", "22bpc_decode_drop_kernelILb1ELb1E")


@pytest.mark.parametrize("key", DROP_KERNELS)
def test_drop_kernels_keep_their_plane_loops_free_of_scratch(device_asm, key):  # noqa: F811
    body = _kernel_body(device_asm, key)
    i0 = next(i for i, ln in enumerate(body) if "v_bcnt_u32_b32" in ln)
    tail = [ln for ln in body[i0:] if re.match(r"^\s*scratch_", ln)]
    assert len(tail) <= 80, f"{key}: {len(tail)} scratch instructions after the first 'v_bcnt_u32_b32'"


def test_drop_kernels_frames_and_registers(device_asm):  # noqa: F811
    name, frames, vgprs = None, {}, {}
    for line in device_asm:
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"^\s*\.amdhsa_private_segment_fixed_size (\d+)", line)
        if m and name and "bpc_decode_drop_kernel" in name:
            frames[name] = int(m.group(1))
        m = re.match(r"^\s*\.amdhsa_next_free_vgpr (\d+)", line)
        if m and name and "bpc_decode_drop_kernel" in name:
            vgprs[name] = int(m.group(1))
    assert len(frames) == 3 and max(frames.values()) <= 192, frames
    assert len(vgprs) == 3 and max(vgprs.values()) <= 64, vgprs          # eight waves a SIMD
