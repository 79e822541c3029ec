"""NumPy statement of 8-bit CLAHE as DESIGN.md section 9g defines it (OpenCV's published clahe.cpp, CPU path, restated): the
definition of record the library's host twin is compared with byte for byte.  It shares no code with the library.

    clahe(img, clip_limit, tiles_x, tiles_y) -> dict(dst, lut, hist, geometry, clipped, batch, residual, ties)
"""
import numpy as np

F = np.float32


def geometry(w, h, clip_limit, tiles_x, tiles_y):
    if w % tiles_x == 0 and h % tiles_y == 0:
        ext_w, ext_h = w, h
    else:                                    # a full tile count more on a side that does divide
        ext_w, ext_h = w + (tiles_x - w % tiles_x), h + (tiles_y - h % tiles_y)
    tile_w, tile_h = ext_w // tiles_x, ext_h // tiles_y
    area = tile_w * tile_h
    clip = 0
    if clip_limit > 0:
        clip = max(min(int(float(clip_limit) * float(area) / 256.0), 2 ** 31 - 1), 1)
    return dict(ext_w=ext_w, ext_h=ext_h, tile_w=tile_w, tile_h=tile_h, clip=clip)


def _reflect(idx, n):
    idx = np.asarray(idx)
    return np.where(idx >= n, 2 * n - 2 - idx, idx)


def _axis(n, tile, tiles):
    """tile indices and float32 weights of every coordinate 0 .. n - 1"""
    inv = F(1.0) / F(tile)
    tf = (np.arange(n).astype(F) * inv).astype(F) - F(0.5)
    fl = np.floor(tf)
    t1 = fl.astype(np.int64)
    a = (tf - fl).astype(F)
    a1 = (F(1.0) - a).astype(F)
    t2 = np.minimum(t1 + 1, tiles - 1)
    t1 = np.maximum(t1, 0)
    return t1, t2, a, a1


def clahe(img, clip_limit=3.0, tiles_x=8, tiles_y=8):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    h, w = img.shape
    g = geometry(w, h, clip_limit, tiles_x, tiles_y)
    tw, th, clip = g["tile_w"], g["tile_h"], g["clip"]
    area = tw * th
    ext = img[_reflect(np.arange(g["ext_h"]), h)][:, _reflect(np.arange(g["ext_w"]), w)]
    hist = np.zeros((tiles_y, tiles_x, 256), dtype=np.int64)
    stats = np.zeros((tiles_y, tiles_x, 3), dtype=np.int64)                 # clipped, batch, residual
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            hs = np.bincount(ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if clip > 0:
                clipped = int(np.maximum(hs - clip, 0).sum())
                hs = np.minimum(hs, clip)
                batch = clipped // 256
                residual = clipped - 256 * batch
                hs = hs + batch
                if residual != 0:
                    step = max(256 // residual, 1)
                    i, served = 0, 0
                    while i < 256 and served < residual:                    # the loop as written, not its closed form
                        hs[i] += 1
                        i += step
                        served += 1
                stats[ty, tx] = (clipped, batch, residual)
            hist[ty, tx] = hs
    scale = F(255.0) / F(area)
    cum = np.cumsum(hist, axis=2)
    lut = np.clip(np.rint((cum.astype(F) * scale).astype(F)), 0, 255).astype(np.uint8)
    tx1, tx2, xa, xa1 = _axis(w, tw, tiles_x)
    ty1, ty2, ya, ya1 = _axis(h, th, tiles_y)
    v = img.astype(np.int64)
    Y1, Y2, X1, X2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    XA, XA1, YA, YA1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    l11, l12 = lut[Y1, X1, v].astype(F), lut[Y1, X2, v].astype(F)
    l21, l22 = lut[Y2, X1, v].astype(F), lut[Y2, X2, v].astype(F)
    top = ((l11 * XA1).astype(F) + (l12 * XA).astype(F)).astype(F)
    bot = ((l21 * XA1).astype(F) + (l22 * XA).astype(F)).astype(F)
    res = ((top * YA1).astype(F) + (bot * YA).astype(F)).astype(F)
    dst = np.clip(np.rint(res), 0, 255).astype(np.uint8)
    fl = np.floor(res)
    ties = int(((res - fl == F(0.5)) & (fl.astype(np.int64) % 2 == 0)).sum())   # round-half-up would give another byte
    return dict(dst=dst, lut=lut, hist=hist.astype(np.int32), geometry=g, clipped=stats[..., 0], batch=stats[..., 1],
                residual=stats[..., 2], ties=ties)
