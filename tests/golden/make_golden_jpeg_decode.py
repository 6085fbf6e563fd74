"""Mints tests/golden/jpeg_decode.npz with Pillow 12 / libjpeg-turbo: JPEG files as Pillow writes them, and the pixels Pillow reads back
from them -- ``Image.open(f).convert('RGB')``, or ``.convert('L')`` for the greyscale files.  Data written by Pillow, nothing else.

    python tests/golden/make_golden_jpeg_decode.py

Keys: ``names``; per name ``file_<name>`` (uint8, the file's bytes), ``rgb_<name>`` (H,W,3) and, for a greyscale file, ``l_<name>`` (H,W).
The 256 x 256 pair (one image with and without restart markers) goes to jpeg_decode_256.npz, which only the GPU test reads."""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def smooth(rng, h, w, ch=3):
    """a low-frequency image with a little noise: something a JPEG of moderate quality keeps structure of"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [127 + 100 * np.sin(x / (3.0 + c) + rng.uniform(0, 6)) * np.cos(y / (4.0 + c) + rng.uniform(0, 6)) + rng.normal(0, 6, (h, w)) for c in range(ch)]
    img = np.clip(np.stack(planes, axis=2), 0, 255).astype(np.uint8)
    return img if ch == 3 else img[:, :, 0]


def noise(rng, h, w, ch=3):
    img = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    return img if ch == 3 else img[:, :, 0]


def save(img, **kw):
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", **kw)
    return f.getvalue()


def cases(rng):
    return [
        ("std_420_q75_17x23", save(smooth(rng, 17, 23), quality=75)),
        ("opt_420_q90_31x18", save(smooth(rng, 31, 18), quality=90, optimize=True)),
        ("opt_444_q60_9x9_noise", save(noise(rng, 9, 9), quality=60, optimize=True, subsampling=0)),
        ("std_422_q85_16x33", save(smooth(rng, 16, 33), quality=85, subsampling=1)),
        ("rst1_420_48x80_noise", save(noise(rng, 48, 80), quality=75, restart_marker_blocks=1)),
        ("rstrow_444_24x24", save(smooth(rng, 24, 24), quality=80, subsampling=0, restart_marker_rows=1)),
        ("grey_q75_13x21", save(smooth(rng, 13, 21, 1), quality=75)),
        ("grey_opt_rst3_33x17", save(smooth(rng, 33, 17, 1), quality=75, optimize=True, restart_marker_blocks=3)),
        ("weblow_20x20", save(smooth(rng, 20, 20), qtables="web_low")),
        ("q1_16x16_noise", save(noise(rng, 16, 16), quality=1)),
        ("q100_8x8_noise", save(noise(rng, 8, 8), quality=100)),
        ("one_pixel", save(noise(rng, 1, 1), quality=75)),
        ("market_128x64_q95", save(smooth(rng, 128, 64), quality=95)),
        ("comment_dpi_12x10", save(smooth(rng, 12, 10), quality=75, comment=b"a comment", dpi=(72, 300))),
    ]


def pixels(out, name, data):
    im = Image.open(io.BytesIO(data))
    out["file_" + name] = np.frombuffer(data, dtype=np.uint8)
    out["rgb_" + name] = np.asarray(im.convert("RGB"))
    if im.mode == "L":
        out["l_" + name] = np.asarray(im.convert("L"))


def main():
    rng = np.random.default_rng(20261020)
    out, names = {}, []
    for name, data in cases(rng):
        names.append(name)
        pixels(out, name, data)
    scans = [bytes(out["file_" + n])[bytes(out["file_" + n]).index(b"\xff\xda"):] for n in names]
    assert any(b"\xff\x00" in s for s in scans), "no file of the set has a stuffed FF"
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "jpeg_decode.npz"), **out)
    big, img = {}, noise(rng, 256, 256)
    for name, kw in (("noise_256", {}), ("noise_256_rstrow", {"restart_marker_rows": 1})):
        pixels(big, name, save(img, quality=100, **kw))
    assert np.array_equal(big["rgb_noise_256"], big["rgb_noise_256_rstrow"])
    del big["rgb_noise_256_rstrow"]
    big["names"] = np.array(["noise_256", "noise_256_rstrow"])
    np.savez_compressed(os.path.join(HERE, "jpeg_decode_256.npz"), **big)
    for f in ("jpeg_decode.npz", "jpeg_decode_256.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
