"""Shared by tests/test_gpu_debug_views.py and tests/test_cpu_debug_images.py: the views k_debug_views (surround360_amd/csrc/
debug_views.hip) is tried on through its test tap (include/s360_debug_views.h), their numpy restatement, and the check itself.

Every combination of: widths 1, 3, 5, 63, 64, 65, 127, 130 (rows of 3 to 520 bytes: below, at and above the 16-byte chunk and the
64-lane wave, odd 3-channel row lengths) plus 1100 (a row of more than one 256-chunk segment); heights 1, 2, 17; shifts 0, 1, w // 3,
w - 1; 0 and 7 rows of padding; 4 -> 4 and 4 -> 3 channels; destinations 0 and 4 bytes behind a 16-byte boundary. Sources are
larger than the rectangle for every other view (a crop at (3, 2)). ALL views go into one call, so most workgroups of the grid (sized
for the largest view) lie past their view's tiles. Every destination is followed by canary bytes."""
import numpy as np

WIDTHS = (1, 3, 5, 63, 64, 65, 127, 130)
HEIGHTS = (1, 2, 17)
PADS = (0, 7)
CHANNELS = (4, 3)
BASES = (0, 4)
CANARY = 0xA5
GAP = 48  # canary bytes behind every destination (then rounded up to the next 16-byte boundary)


def views():
    out = []
    k = 0
    sizes = [(w, h) for w in WIDTHS for h in HEIGHTS] + [(1100, 3)]
    for w, h in sizes:
        for shift in sorted({0, 1 % w, w // 3, w - 1}):
            for pad in PADS:
                for cout in CHANNELS:
                    for base in BASES:
                        crop = k % 2 == 1
                        out.append(dict(w=w, h=h, shift=shift, pad_rows=pad, channels_out=cout, base=base,
                                        x0=3 if crop else 0, y0=2 if crop else 0,
                                        src_pitch=w + (5 if crop else 0), src_rows=h + (3 if crop else 0)))
                        k += 1
    return out


def layout(vs, seed=5):
    """(tap views, source area, destination area as handed in, destination area expected)."""
    rng = np.random.default_rng(seed)
    taps, srcs = [], []
    src_off = dst_off = 0
    spans = []
    for v in vs:
        img = rng.integers(0, 256, (v["src_rows"], v["src_pitch"], 4), dtype=np.uint8)
        srcs.append(img)
        n_dst = v["w"] * (v["h"] + v["pad_rows"]) * v["channels_out"]
        at = dst_off + v["base"]
        taps.append(dict(src_off=src_off, dst_off=at, src_pitch=v["src_pitch"], src_rows=v["src_rows"], x0=v["x0"], y0=v["y0"],
                         w=v["w"], h=v["h"], shift=v["shift"], pad_rows=v["pad_rows"], channels_in=4, channels_out=v["channels_out"]))
        spans.append((at, n_dst))
        src_off += (img.size + 15) // 16 * 16
        dst_off = (at + n_dst + GAP + 15) // 16 * 16
    src = np.zeros(src_off, np.uint8)
    dst = np.full(dst_off, CANARY, np.uint8)
    want = dst.copy()
    for v, t, img, (at, n_dst) in zip(vs, taps, srcs, spans):
        src[t["src_off"]:t["src_off"] + img.size] = img.ravel()
        want[at:at + n_dst] = restate(img, v).ravel()
    return taps, src, dst, want


def restate(img, v):
    """crop, np.roll, zero pad, drop alpha."""
    rect = img[v["y0"]:v["y0"] + v["h"], v["x0"]:v["x0"] + v["w"]]
    out = np.roll(rect, v["shift"], axis=1)
    out = np.concatenate([out, np.zeros((v["pad_rows"], v["w"], 4), np.uint8)], axis=0)
    return np.ascontiguousarray(out[:, :, :v["channels_out"]])


def check_all(ctx):
    from surround360_amd import debug_images as DI
    vs = views()
    assert len(vs) > 600 and {v["w"] * v["channels_out"] % 16 for v in vs} - {0}, "the cases lost their odd row lengths"
    taps, src, dst, want = layout(vs)
    got = DI.debug_views(ctx, taps, src, dst)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        first = int(bad[0])
        k = max(i for i, t in enumerate(taps) if t["dst_off"] <= first) if first >= taps[0]["dst_off"] else 0
        raise AssertionError("%d bytes differ, the first at %d: view %d %r (+%d): got %d, want %d (canary %d)" % (
            bad.size, first, k, vs[k], first - taps[k]["dst_off"], got[first], want[first], CANARY))
