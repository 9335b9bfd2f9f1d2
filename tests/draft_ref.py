"""Pillow as the reference of a drafted decode, for the draft tests.

``draft_at(im, mode, s)`` makes Pillow decode ``im`` at libjpeg scale 1/s. Where
``Image.draft`` can pick that scale (both sides at least ``s`` pixels) it is
asked to, with the request ``(W // s, H // s)``; an image smaller than ``s`` on
a side never gets that scale from ``draft`` (its rule is ``min(W // w, H //
h)``), so there the same three fields ``draft`` sets (the tile's extent, the
size and ``decoderconfig``) are set to the scale directly, and Pillow's decoder
runs libjpeg at it all the same. Either way the resulting size is asserted.
"""
import io

import numpy as np


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def draft_at(im, mode: str, s: int):
    from PIL import ImageFile

    W, H = im.size
    want = (ceil_div(W, s), ceil_div(H, s))
    if s == 1:
        im.draft(mode, None)
    elif W >= s and H >= s:
        im.draft(mode, (W // s, H // s))
    else:
        im.draft(mode, None)  # the mode, scale 1
        d, e, o, a = im.tile[0]
        im.tile = [ImageFile._Tile(d, (e[0], e[1], e[0] + want[0], e[1] + want[1]), o, a)]
        im._size = want
        im.decoderconfig = (s, 0)
    assert im.size == want and im.decoderconfig[0] == s, (im.size, im.decoderconfig, want, s)
    return im


def drafted_rgb(data: bytes, s: int):
    """The PIL image (mode RGB) of ``data`` decoded at scale 1/s."""
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    W, H = im.size
    out = draft_at(im, "RGB", s).convert("RGB")
    assert out.size == (ceil_div(W, s), ceil_div(H, s))
    return out


def drafted_array(data: bytes, s: int) -> np.ndarray:
    return np.asarray(drafted_rgb(data, s))
