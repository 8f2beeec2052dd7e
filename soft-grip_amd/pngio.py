"""Minimal PNG writer (standard library only: zlib + struct): 8-bit RGB or RGBA, no filtering."""
import struct
import zlib

import numpy as np


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def encode_png(img):
    """uint8 array [H, W, 3] (RGB) or [H, W, 4] (RGBA) -> PNG file bytes"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] not in (3, 4):
        raise ValueError("encode_png wants an [H, W, 3|4] uint8 image, got %s" % (img.shape,))
    h, w, c = img.shape
    raw = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * c)], axis=1).tobytes()   # filter byte 0 per row
    header = struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 6, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", header) + _chunk(b"IDAT", zlib.compress(raw, 6)) + _chunk(b"IEND", b"")


def write_png(path, img):
    with open(path, "wb") as f:
        f.write(encode_png(img))
