"""Text deflated on the device into BGZF members, opt-in: the ``gf_df_*`` calls of libgfdeflate.so
(include/gf_deflate.h, which states the format).

The counterpart of ``bgzf``'s device inflate: the FASTQ text ``read_write`` formats in HBM is cut into members of
``TEXT`` bytes, each deflated by one workgroup — LZ77 tokens under dynamic Huffman codes, or stored when that is not
longer — and the members leave the device back to back, ready to be written as they are.  With ``EOF_MARKER`` behind
them they are a file bgzip, htslib and this project's own ``inflate="device"`` read member by member.  A member's bytes
are a function of its text alone: ``deflate_member_host`` gives the same member on the host, without a GPU.
libgfdeflate.so is a library of its own next to libgfmatch.so (genefuserust_amd/scan_csrc/).  No CPU fallback for the
device call: without the library and a GPU it raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from . import _lib

DF_LIB_PATH = os.path.join(_lib._HERE, "libgfdeflate.so")

TEXT = 65280          # text bytes per member: GF_DF_TEXT_BYTES
STORED_OVER = 31      # what a stored member is longer than its text
TOTALS = 5            # members, text bytes, compressed bytes, members stored, members under dynamic codes
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

_vp, _i64 = C.c_void_p, C.c_int64

# libgfdeflate.so, loaded (once) after libgfmatch.so.  Raises if it has not been built.
lib, check = _lib.companion(DF_LIB_PATH, "device deflate", "gf_df_last_error", {
    "gf_df_members": (_i64, [_i64]),
    "gf_df_out_cap": (_i64, [_i64]),
    "gf_df_workspace_bytes": (_i64, [_i64]),
    "gf_df_deflate_device": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "gf_df_member_host": (C.c_int, [_vp, _i64, _vp, _i64, C.POINTER(_i64)]),
    "gf_df_last_error": (C.c_char_p, []),
})


def members(text_cap: int) -> int:
    """The members ``text_cap`` bytes of text make at most."""
    return max(0, -(-int(text_cap) // TEXT))


def out_cap(text_cap: int) -> int:
    """What the members of ``text_cap`` bytes of text can never pass."""
    return max(0, int(text_cap)) + STORED_OVER * members(text_cap)


def deflate_device(text, text_bytes=None, stream=None):
    """``text`` (a uint8 device tensor, any alignment) deflated into BGZF members: (out, member_off, totals).
    ``text_bytes``: an int64 device tensor of one element, the true length of the text, read on the device — the
    members past it are absent; None: all of ``text``.  ``out``: a uint8 device tensor of the capacity, of which
    ``member_off[-1]`` bytes are members, back to back; ``member_off``: int64[members + 1]; ``totals``: the int64[5]
    device tensor of this call (members, text bytes, compressed bytes, members stored, members under dynamic codes).
    Asynchronous: nothing is read back."""
    import torch
    _lib.need_device_tensors("deflate_device", text, *(() if text_bytes is None else (text_bytes,)))
    assert text.dtype == torch.uint8 and text.dim() == 1 and text.is_contiguous()
    if text_bytes is not None:
        assert text_bytes.dtype == torch.int64 and text_bytes.numel() == 1 and text_bytes.device == text.device
    dev, cap = text.device, int(text.numel())
    L = lib()
    n_members, o_cap, ws_bytes = members(cap), out_cap(cap), int(L.gf_df_workspace_bytes(cap))
    out = torch.empty(max(o_cap, 1), dtype=torch.uint8, device=dev)
    member_off = torch.zeros(n_members + 1, dtype=torch.int64, device=dev)
    totals = torch.zeros(TOTALS, dtype=torch.int64, device=dev)
    ws = _lib.workspace(ws_bytes, dev, stream)
    check(L.gf_df_deflate_device(text.data_ptr() if cap else None, cap,
                                 None if text_bytes is None else text_bytes.data_ptr(), out.data_ptr(), o_cap,
                                 member_off.data_ptr(), totals.data_ptr(), ws.data_ptr(), ws_bytes,
                                 _lib.stream_handle(dev, stream)))
    for t in (out, member_off, totals, text) + (() if text_bytes is None else (text_bytes,)):
        _lib.for_stream(t, stream)
    return out, member_off, totals


def deflate_member_host(data) -> bytes:
    """The member the device writes for ``data`` (1 .. ``TEXT`` bytes), computed on the host: no GPU."""
    data = bytes(data)
    if not 1 <= len(data) <= TEXT:
        raise ValueError("deflate_member_host takes 1 .. %d bytes of text, not %d" % (TEXT, len(data)))
    out = C.create_string_buffer(len(data) + STORED_OVER)
    size = _i64(0)
    check(lib().gf_df_member_host(data, len(data), out, len(out), C.byref(size)))
    return out.raw[:size.value]


def deflate_host(data) -> bytes:
    """The members of ``data`` of any length, back to back, as ``deflate_device`` leaves them (without the marker)."""
    data = bytes(data)
    return b"".join(deflate_member_host(data[k:k + TEXT]) for k in range(0, len(data), TEXT))
