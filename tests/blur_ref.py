"""numpy restatement of PIL's BoxBlur / GaussianBlur for 8-bit images (Pillow 12.2 BoxBlur.c), in two forms that must agree byte for byte:

  line_window    out[x] = (ww * sum_{i=-r..r} in[clamp(x+i)] + fw * (in[clamp(x-r-1)] + in[clamp(x+r+1)]) + 2^23) >> 24, the form the kernels compute
  line_running   PIL's literal loop: a running accumulator, edgeA = min(r+1, size), edgeB = max(size-r-1, 0)

Integer sums are associative, so the two give the same bytes, lines shorter than r + 1 included. The constants (r, ww, fw) come in from the caller:
the tests pass unigen_amd.image's own `box_blur_constants` / `gaussian_box_radius`, so these are pinned against PIL together with the arithmetic.
Images are uint8 arrays [B, H, W, C]; `consts` is ((rx, wwx, fwx), (ry, wwy, fwy)), an axis whose entry is None is skipped (PIL skips a zero radius).
"""
import numpy as np

HALF = 1 << 23

# ---- the cases of tests/golden/blur_tiny.safetensors (written by tests/golden/make_blur_golden.py) ---------------------------------------------------
# sizes around the box radius r = 9 of GaussianBlur(10), its reach r + 1 = 10 and the halo of three passes, 30
SIZES = [(1, 1), (3, 200), (7, 5), (10, 10), (19, 20), (21, 22), (31, 29), (40, 50), (64, 300), (300, 64)]
MORE_ON = [(7, 5), (40, 50)]           # the sizes that also carry the other radii, the tuple radii and BoxBlur
GAUSS = {"g0.5": 0.5, "g1": 1, "g3.7": 3.7, "g25": 25, "g10x0": (10, 0), "g0x10": (0, 10), "g3x7.5": (3, 7.5)}
BOX = {"b0.5": 0.5, "b2": 2, "b9.475": 9.475}


def filters(H, W):
    """name -> ("gaussian" | "box", radius) of every stored output of an H x W input."""
    out = {"g10": ("gaussian", 10)}
    if (H, W) in MORE_ON:
        out.update({k: ("gaussian", v) for k, v in GAUSS.items()})
        out.update({k: ("box", v) for k, v in BOX.items()})
    return out


def bw_image(H, W):
    """The seeded image of size H x W whose bytes are all 0 or 255, uint8 [H, W, 3] (the fixture stores its SHA-256, not its bytes)."""
    return (np.random.default_rng(400 + SIZES.index((H, W))).integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)


def line_window(lines, r, ww, fw):
    """lines uint8 [N, size, ...]: one pass along axis 1, the clamped direct window."""
    size = lines.shape[1]
    src = lines.astype(np.uint32)
    idx = np.arange(size)
    at = lambda off: src[:, np.clip(idx + off, 0, size - 1)]
    acc = np.zeros_like(src)
    for i in range(-r, r + 1):
        acc += at(i)
    bulk = acc * np.uint32(ww) + (at(-r - 1) + at(r + 1)) * np.uint32(fw) + np.uint32(HALF)
    return (bulk >> np.uint32(24)).astype(np.uint8)


def line_running(lines, r, ww, fw):
    """The same pass as BoxBlur.c's ImagingLineBoxBlur8 writes it: one accumulator that slides along the line."""
    size = lines.shape[1]
    last = size - 1
    src = lines.astype(np.uint32)
    out = np.empty_like(src)
    ww, fw = np.uint32(ww), np.uint32(fw)
    edge_a, edge_b = min(r + 1, size), max(size - r - 1, 0)
    save = lambda x, acc, left, right: out.__setitem__((slice(None), x), (acc * ww + (src[:, left] + src[:, right]) * fw + np.uint32(HALF)) >> np.uint32(24))
    acc = src[:, 0] * np.uint32(r + 1)                       # the window of x = -1
    for x in range(0, edge_a - 1):
        acc = acc + src[:, x]
    acc = acc + src[:, last] * np.uint32(r - edge_a + 1)     # a line shorter than the radius: the rest is the last pixel
    if edge_a <= edge_b:
        for x in range(0, edge_a):                           # left edge: pixel 0 leaves, x + r enters
            acc = acc + src[:, x + r] - src[:, 0]
            save(x, acc, 0, x + r + 1)
        for x in range(edge_a, edge_b):
            acc = acc + src[:, x + r] - src[:, x - r - 1]
            save(x, acc, x - r - 1, x + r + 1)
        for x in range(edge_b, size):                        # right edge: the last pixel enters
            acc = acc + src[:, last] - src[:, x - r - 1]
            save(x, acc, x - r - 1, last)
    else:
        for x in range(0, edge_b):
            acc = acc + src[:, x + r] - src[:, 0]
            save(x, acc, 0, x + r + 1)
        for x in range(edge_b, edge_a):                      # both ends of the window are outside the line
            acc = acc + src[:, last] - src[:, 0]
            save(x, acc, 0, last)
        for x in range(edge_a, size):
            acc = acc + src[:, last] - src[:, x - r - 1]
            save(x, acc, x - r - 1, last)
    return out.astype(np.uint8)


def box_blur(img, consts, passes=1, line=line_window):
    """`passes` passes along rows, then `passes` along columns, uint8 after every pass. img [B, H, W, C]."""
    cx, cy = consts
    out = img
    if cx is not None:
        t = out.reshape(-1, out.shape[2], out.shape[3])                                    # [B * H, W, C]
        for _ in range(passes):
            t = line(t, *cx)
        out = t.reshape(out.shape)
    if cy is not None:
        B, H, W, C = out.shape
        t = out.transpose(0, 2, 1, 3).reshape(B * W, H, C)                                 # [B * W, H, C]
        for _ in range(passes):
            t = line(t, *cy)
        out = t.reshape(B, W, H, C).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(out)
