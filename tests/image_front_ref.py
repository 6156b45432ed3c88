"""Host reference of the uint8 image fronts (``csrc/image_front.hip``) in plain torch on the CPU: ToTensor + Normalize in fp32, one rounding
to the storage type.  The kernels are held bit-equal to it: the build has no fast-math, the fp32 divide is correctly rounded and both sides
apply the same three operations in the same order."""
import torch


def normalise(u8, mean=0.5, std=0.5):
    return (u8.float() / 255 - mean) / std


def nhwc_rows(u8, dtype, mean=0.5, std=0.5):
    """uint8 [n, H, W, C] -> [n H W, C]"""
    return normalise(u8, mean, std).reshape(-1, u8.shape[-1]).to(dtype)


def patch_rows(u8, ps, dtype, mean=0.5, std=0.5):
    """uint8 [n, R, R, C] -> the im2col rows [n G G, C ps ps], G = R / ps, columns ordered (c, i, j)"""
    n, R, _, C = u8.shape
    G = R // ps
    return normalise(u8, mean, std).view(n, G, ps, G, ps, C).permute(0, 1, 3, 5, 2, 4).reshape(n * G * G, C * ps * ps).to(dtype)


def keep_rows(rows, keep, n_patches):
    """A row gather of the im2col rows: ``rows`` [n n_patches, K], ``keep`` int [n, len_keep] -> [n len_keep, K]; an entry outside
    [0, n_patches) gives a zero row."""
    n, K = keep.shape[0], rows.shape[1]
    keep = keep.long().to(rows.device)
    ok = (keep >= 0) & (keep < n_patches)
    idx = torch.arange(n, device=rows.device)[:, None] * n_patches + keep.clamp(0, n_patches - 1)
    out = rows[idx.reshape(-1)].clone()
    out[~ok.reshape(-1)] = 0
    return out.reshape(n * keep.shape[1], K)
