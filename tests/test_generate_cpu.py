"""Host side of generator inference (no GPU): the PNG encoder, the latent helpers, the generate CLI's parser and plan, the
chunk plan of DcganEngine.sample, and the sampler's refusal to run without a device."""
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jck-generation_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)


def _decode_png(data):
    """the inverse of the encoder, for the subset it writes: 8-bit grey / RGB, filter type 0, any number of IDAT chunks"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (0, 2)
    ch = 3 if colour == 2 else 1
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), np.uint8).reshape(h, 1 + w * ch)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape((h, w, 3) if ch == 3 else (h, w))


@pytest.mark.parametrize("shape", [(1, 1, 3), (5, 7, 3), (64, 130, 3), (9, 4)])
def test_png_round_trip(shape):
    from train.gan_trainer import _encode_png
    img = np.random.default_rng(1).integers(0, 256, shape, dtype=np.uint8)
    data = _encode_png(img)
    assert np.array_equal(_decode_png(data), img)
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.array(Image.open(io.BytesIO(data))), img)


def test_png_rejects_other_input():
    from train.gan_trainer import _encode_png
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            _encode_png(bad)


def test_slerp():
    from hipgan.sampler import slerp
    g = torch.Generator().manual_seed(0)
    z0, z1 = torch.randn(100, generator=g), torch.randn(100, generator=g)
    z1 = z1 * (z0.norm() / z1.norm())
    p = slerp(z0, z1, 9)
    assert p.shape == (9, 100) and torch.equal(p[0], z0) and torch.equal(p[-1], z1)
    assert torch.allclose(p.norm(dim=1), z0.norm().expand(9), rtol=1e-5)             # equal norms: the whole arc keeps it
    mid = (z0 + z1) / (z0 + z1).norm() * z0.norm()
    assert torch.allclose(p[4], mid, atol=1e-5)
    assert torch.equal(slerp(z0, z0, 3), z0.expand(3, 100))                           # degenerate: the straight line
    with pytest.raises(Exception):
        slerp(z0, z1, 1)


def test_latents_and_truncation():
    from hipgan.sampler import latents
    a, b = latents(64, 3), latents(64, 3)
    assert a.shape == (64, 100) and a.dtype == torch.float32 and torch.equal(a, b) and not torch.equal(a, latents(64, 4))
    assert float(a.abs().max()) > 2.5                                                # untruncated
    t = latents(64, 3, truncation=0.7)
    assert float(t.abs().max()) <= 0.7 and float(t.abs().max()) > 0.6 and torch.equal(t, latents(64, 3, truncation=0.7))
    with pytest.raises(Exception):
        latents(4, 0, truncation=0.0)


def test_checkpoint_selection():
    from hipgan import JckError
    from hipgan.sampler import image_size_of, one_hot, pick_generator_state
    live, ema = {"conv1.weight": 1}, {"conv1.weight": 2}
    assert pick_generator_state({"model_g": live}, "auto") == (live, "live")
    assert pick_generator_state({"model_g": live, "model_g_ema": ema}, "auto") == (ema, "ema")
    assert pick_generator_state({"model_g": live, "model_g_ema": ema}, "live") == (live, "live")
    for ckpt, which in (({"model_g": live}, "ema"), ({}, "auto"), ({"model_g": live}, "best")):
        with pytest.raises(JckError):
            pick_generator_state(ckpt, which)
    assert image_size_of({f"conv{i}.weight": 0 for i in range(1, 6)}) == 64
    assert image_size_of({f"conv{i}.weight": 0 for i in range(1, 7)}) == 128
    oh = one_hot([3, 17])
    assert oh.shape == (2, 100) and oh.dtype == torch.int64 and oh[0, 3] == 1 and oh[1, 17] == 1 and int(oh.sum()) == 2
    with pytest.raises(JckError):
        one_hot([100])


def test_chunk_plan():
    from hipgan.engine import chunk_plan
    assert chunk_plan(20, 8) == [(0, 8), (8, 16), (16, 20)]
    assert chunk_plan(8, 8) == [(0, 8)] and chunk_plan(1, 8) == [(0, 1)] and chunk_plan(9, 8) == [(0, 8), (8, 9)]
    assert chunk_plan(0, 8) == []
    with pytest.raises(Exception):
        chunk_plan(4, 0)


def test_cli_parser_and_plan():
    import generate
    a = generate.get_arg_parse(["--checkpoint", "c.pt", "--out", "o"])
    assert generate.get_arg_parse(["--checkpoint", "c.pt", "--out", "o", "--interpolate", "2:5"]).num == 64
    assert (a.model, a.num, a.batch_size, a.seed, a.bn, a.which, a.calibrate, a.truncation, a.classes, a.interpolate) == \
        ("DCGAN", 64, 64, 0, "running", "auto", 0, None, None, None)
    a = generate.get_arg_parse(["-m", "CGAN", "--checkpoint", "c.pt", "--num", "3", "-b", "8", "--seed", "5", "--truncation", "0.5", "--bn", "batch",
                                "--which", "ema", "--calibrate", "2", "--classes", "3,17", "--out", "o"])
    assert (a.model, a.num, a.batch_size, a.seed, a.truncation, a.bn, a.which, a.calibrate, a.classes) == ("CGAN", 3, 8, 5, 0.5, "batch", "ema", 2, [3, 17])
    z, cls, per_row = generate.plan(a)
    assert z.shape == (6, 100) and float(z.abs().max()) <= 0.5 and cls.tolist() == [3, 3, 3, 17, 17, 17] and per_row == 3     # a row per class
    a = generate.get_arg_parse(["--checkpoint", "c.pt", "--out", "o", "--interpolate", "2:5"])
    z, cls, per_row = generate.plan(a)
    assert a.interpolate == (2, 5) and z.shape == (10, 100) and cls is None and per_row == 5
    assert not torch.equal(z[0], z[5]) and not torch.equal(z[0], z[4])
    a = generate.get_arg_parse(["--checkpoint", "c.pt", "--out", "o", "--num", "20"])
    z, cls, per_row = generate.plan(a)
    assert z.shape == (20, 100) and cls is None and torch.equal(z, generate.plan(a)[0])
    for bad in (["--out", "o"], ["--checkpoint", "c", "--out", "o", "--num", "0"], ["--checkpoint", "c", "--out", "o", "--classes", "3"],
                ["-m", "CGAN", "--checkpoint", "c", "--out", "o", "--classes", "3,100"], ["--checkpoint", "c", "--out", "o", "--interpolate", "2"],
                ["--checkpoint", "c", "--out", "o", "--interpolate", "1:1"], ["--checkpoint", "c", "--out", "o", "--bn", "eval"],
                ["--checkpoint", "c", "--out", "o", "--truncation", "0"], ["--checkpoint", "c", "--out", "o", "--interpolate", "2:5", "--num", "8"]):
        with pytest.raises(SystemExit):
            generate.get_arg_parse(bad)
    a = generate.get_arg_parse(["-m", "CGAN", "--checkpoint", "c.pt", "--out", "o", "--interpolate", "3:4", "--classes", "3,17"])
    z, cls, per_row = generate.plan(a)                    # interpolation rows cycle through the classes
    assert z.shape == (12, 100) and cls.tolist() == [3] * 4 + [17] * 4 + [3] * 4 and per_row == 4
    a = generate.get_arg_parse(["-m", "CGAN", "--checkpoint", "c.pt", "--out", "o", "--num", "5"])
    cls = generate.plan(a)[1]
    assert cls.shape == (5,) and int(cls.min()) >= 0 and int(cls.max()) < 100
    sheet = generate.grid_u8(np.full((5, 4, 4, 3), 200, np.uint8), 3)
    assert sheet.shape == (14, 20, 3) and sheet.dtype == np.uint8 and sheet[2, 2, 0] == 200 and sheet[0, 0, 0] == 0 and sheet[8, 14, 0] == 0


def test_sampler_needs_a_gpu(monkeypatch):
    from hipgan import JckError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from hipgan.sampler import Sampler
    with pytest.raises(JckError, match="needs a GPU"):
        Sampler.from_checkpoint({"model_g": {f"conv{i}.weight": torch.zeros(1) for i in range(1, 6)}}, "DCGAN")
    with pytest.raises(JckError, match="DCGAN"):
        Sampler.from_checkpoint({"model_g": {}}, "WGAN")
