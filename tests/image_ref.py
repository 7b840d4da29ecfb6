"""numpy restatements of the image front end's kernels (unigen_amd/csrc/image.hip): one right answer per element, compared with equality.

  canny_grad / canny_nms / canny_hysteresis / canny     cv::Canny with L2gradient = false, restated from OpenCV's published source (canny.cpp); no vectors of
                                                        cv2.Canny exist here ("parity unpinned") - tests/test_image_ref_cpu.py checks the
                                                        stages against independent scipy / naive-loop implementations
  resample_tables / resize                              PIL's ImagingResample for 8-bit images with the LANCZOS filter (Resample.c: precompute_coeffs,
                                                        normalize_coeffs_8bpc, the horizontal / vertical 8bpc passes), pinned against PIL itself
  rgb_to_l                                              PIL's convert("L")
  u8_to_chw / chw_to_u8                                 diffusers' VaeImageProcessor: pil_to_numpy + normalize, denormalize + numpy_to_pil
Images are uint8 arrays [B, H, W, C].
"""
import math

import numpy as np
import torch

TG22, CANNY_SHIFT = 13573, 15
PRECISION_BITS = 32 - 8 - 2


# ---- Canny -----------------------------------------------------------------------------------------------------------------------------------------
def sobel(img):
    """img [B, H, W, C] uint8 -> (dx, dy) int32 per channel, replicated borders (cv::Sobel ksize 3, BORDER_REPLICATE)."""
    p = np.pad(img.astype(np.int32), ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = img.shape[1:3]
    s = lambda dy, dx: p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    dx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    dy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    return dx, dy


def canny_grad(img):
    """-> dx, dy (int16), mag (int32), each [B, H, W]: per pixel the channel with the largest |dx| + |dy|, the first one on a tie."""
    dx, dy = sobel(img)
    mag = np.abs(dx) + np.abs(dy)
    best = np.argmax(mag, axis=-1)[..., None]            # argmax returns the FIRST maximum: OpenCV's strict >
    take = lambda a: np.take_along_axis(a, best, axis=-1)[..., 0]
    return take(dx).astype(np.int16), take(dy).astype(np.int16), take(mag).astype(np.int32)


def canny_nms(dx, dy, mag, low, high):
    """-> map uint8 [B, H, W]: 2 strong, 0 candidate, 1 not an edge."""
    if low > high:
        low, high = high, low
    xs, ys, m = dx.astype(np.int64), dy.astype(np.int64), mag.astype(np.int64)
    B, H, W = m.shape
    p = np.pad(m, ((0, 0), (1, 1), (1, 1)))               # magnitudes outside the image are 0
    nb = lambda oy, ox: p[:, 1 + oy:1 + oy + H, 1 + ox:1 + ox + W]
    x, y = np.abs(xs), np.abs(ys) << CANNY_SHIFT
    tg22x = x * TG22
    tg67x = tg22x + (x << (CANNY_SHIFT + 1))
    horiz = y < tg22x
    vert = ~horiz & (y > tg67x)
    diag = ~horiz & ~vert
    neg = (xs ^ ys) < 0                                   # s = -1: compare with up-right and down-left
    keep_h = (m > nb(0, -1)) & (m >= nb(0, 1))
    keep_v = (m > nb(-1, 0)) & (m >= nb(1, 0))
    keep_d = np.where(neg, (m > nb(-1, 1)) & (m > nb(1, -1)), (m > nb(-1, -1)) & (m > nb(1, 1)))
    keep = (m > low) & ((horiz & keep_h) | (vert & keep_v) | (diag & keep_d))
    out = np.ones((B, H, W), np.uint8)
    out[keep] = 0
    out[keep & (m > high)] = 2
    return out


def canny_hysteresis(emap):
    """Promote candidates 8-connected to a strong pixel (breadth-first, a stack as in OpenCV) -> uint8 255 / 0."""
    emap = emap.copy()
    B, H, W = emap.shape
    for b in range(B):
        m = emap[b]
        stack = list(zip(*np.nonzero(m == 2)))
        while stack:
            y, x = stack.pop()
            for oy in (-1, 0, 1):
                for ox in (-1, 0, 1):
                    yy, xx = y + oy, x + ox
                    if 0 <= yy < H and 0 <= xx < W and m[yy, xx] == 0:
                        m[yy, xx] = 2
                        stack.append((yy, xx))
    return np.where(emap == 2, 255, 0).astype(np.uint8)


def canny(img, low=100, high=200):
    """cv2.Canny(img, low, high) of every image of a batch [B, H, W, C] -> [B, H, W] uint8."""
    dx, dy, mag = canny_grad(img)
    return canny_hysteresis(canny_nms(dx, dy, mag, low, high))


# ---- PIL resampling ----------------------------------------------------------------------------------------------------------------------------------
def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def resample_tables(in_size, out_size):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc -> (bounds int32 [out, 2] = (first, taps), coef int32 [out, ksize], ksize). float64 as in C."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):                          # (int)(+-0.5 + v * 2^22): truncation toward zero = round half away
            coef[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return bounds, coef, ksize


def _resample_axis(img, out_size, axis):
    bounds, coef, _ = resample_tables(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for o in range(out_size):
        first, n = bounds[o]
        k = coef[o, :n].astype(np.int64).reshape((n,) + (1,) * (src.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (src[first:first + n] * k).sum(0)
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, out_h, out_w):
    """PIL Image.resize((out_w, out_h), LANCZOS) of [B, H, W, C] uint8: horizontal pass, then vertical, uint8 between them; unchanged sizes are skipped."""
    if img.shape[2] != out_w:
        img = _resample_axis(img, out_w, 2)
    if img.shape[1] != out_h:
        img = _resample_axis(img, out_h, 1)
    return img


def rgb_to_l(img):
    """PIL convert("L"): [B, H, W, 3] -> [B, H, W, 1]."""
    v = img.astype(np.uint32)
    return ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16).astype(np.uint8)[..., None]


# ---- converters --------------------------------------------------------------------------------------------------------------------------------------
def u8_to_chw(img, normalize=True, dtype=torch.float32, replicate=False):
    """[B, H, W, C] uint8 -> torch [B, C (3 when a gray image is replicated), H, W]: v / 255 then 2 x - 1, each rounded in fp32; bf16 rounds that value."""
    x = img.astype(np.float32) / np.float32(255.0)
    if normalize:
        x = np.float32(2.0) * x - np.float32(1.0)
    t = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))
    if replicate and t.shape[1] == 1:
        t = t.repeat(1, 3, 1, 1)
    return t.to(dtype)


def chw_to_u8(x):
    """torch [B, C, H, W] fp32 / bf16 -> uint8 [B, H, W, C]: (x * 0.5 + 0.5) in x's dtype, clamp, fp32, * 255, round half to even."""
    half = torch.tensor(0.5, dtype=x.dtype)
    t = ((x * half) + half).clamp(0, 1).float().numpy()
    return np.rint(t * np.float32(255.0)).astype(np.uint8).transpose(0, 2, 3, 1)


# ---- seeded test images --------------------------------------------------------------------------------------------------------------------------------
def synth(B, H, W, C, seed=0, levels=None):
    """Smooth blobs + hard edges + noise; `levels` quantises to that many grey levels (plateaus: ties in NMS, equal channels, exact thresholds)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((B, H, W, C))
    for b in range(B):
        for c in range(C):
            v = np.zeros((H, W))
            for _ in range(3):
                cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(2, 4 + max(H, W) / 3)
                v += rng.uniform(60, 160) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            y0, x0 = rng.integers(0, H), rng.integers(0, W)
            v[y0:y0 + max(1, H // 3), x0:x0 + max(1, W // 3)] += rng.uniform(80, 200)        # a rectangle: hard edges
            v[(yy + xx * rng.uniform(0.3, 2)) % rng.uniform(9, 23) < 2] += 90                  # slanted stripes
            v += rng.normal(0, 6, (H, W))
            out[b, :, :, c] = v
        if C == 3 and levels is not None:
            out[b, :, :, 1] = out[b, :, :, 0]              # two equal channels: channel ties everywhere they win
    out = np.clip(out, 0, 255)
    if levels is not None:
        # steps of 25 or 50: |dx| + |dy| takes multiples of 25, so magnitudes land exactly on thresholds of 100 and 200
        out = np.floor(out / 256 * levels) * (50 if levels <= 4 else 25)
    return np.clip(out, 0, 255).astype(np.uint8)
