"""numpy oracle of wun_gather_snippets (include/wun.h): a descriptor table [B, S] of (start, gain, flags) turned into a batch
with float32 products and ascending float32 adds, indexing per source -- no shared code with the kernel or the producers."""
import numpy as np

SWAP, NEGATE = 1, 2


def source_window(plane, rec, t_in):
    """a_s of the contract: gain * plane[start : start + t_in][c'], sign flipped on request; gain 1 leaves the bits alone."""
    start, gain, flags = int(rec["start"]), np.float32(rec["gain"]), int(rec["flags"])
    x = plane[start:start + t_in, :]
    assert x.shape[0] == t_in, "window outside the plane"
    if flags & SWAP:
        x = x[:, ::-1]
    a = x.copy() if gain == np.float32(1.0) else (gain * x).astype(np.float32)
    if flags & NEGATE:
        a = -a
    return a


def gather(planes, mix_plane, table, mix_mode, t_in, t_out):
    """(mix [B, t_in, C], targets [S, B, t_out, C], windows [S, B, t_in, C]) of table [B, S]; planes: S arrays [N, C]."""
    B, S = table.shape
    pad = (t_in - t_out) // 2
    win = np.stack([np.stack([source_window(planes[s], table[b, s], t_in) for b in range(B)]) for s in range(S)])
    if mix_mode:
        mix = win[0].copy()
        for s in range(1, S):
            mix = (mix + win[s]).astype(np.float32)
    else:
        mix = np.stack([mix_plane[int(table[b, 0]["start"]):int(table[b, 0]["start"]) + t_in, :] for b in range(B)])
    return mix, np.ascontiguousarray(win[:, :, pad:pad + t_out, :]), win
