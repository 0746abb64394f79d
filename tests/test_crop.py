"""Cropped display output on the GPU (crop.hip): the SPS crop window as packed
I420 in the layout of the reference testbench's CropPicture
(DecTestBench.c:588-666), or as RGBA.

Pinned by tests/golden/crop.json (tests/golden/make_crop_golden.py: the
reference testbench run with -C on generated streams).  Every comparison is
exact equality."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import _crop
import _golden
from broadway_amd import gen
from broadway_amd.decoder import Decoder, split_annexb

ROOT = _crop.ROOT
CASES = _crop.cases()
SMALL = ["crop_ltrb_6x4", "crop_r_16x3"]


def case_stream(name):
    c = CASES[name]
    s = gen.generate(c["config"], c["seed"], **c["overrides"])
    assert hashlib.sha256(s).hexdigest() == c["stream_sha256"], "generator drift"
    return s


def head_nals(stream, case):
    """The NAL units of the pictures the fixture records (all of a small
    stream; SPS + PPS + the first pictures' slices of a long one)."""
    nals = split_annexb(stream)
    if len(case["frames"]) == case["frames_total"]:
        return nals
    slices = case["overrides"].get("slices", 4)
    return nals[:2 + slices * len(case["frames"])]


@pytest.fixture(scope="module", autouse=True)
def _leave_the_engine_pool_empty():
    """The decoder instances of the GPU tests here leave engines of four
    picture sizes in the library's pool of released engines (four entries,
    each kept until an instance of its size takes it).
    tests/test_gpu_parity.py::test_swdec_pooled_engines_vs_reference, which
    runs later, counts the engines its own 11x9 instances reuse, and a pool
    full of other sizes gives it none: drain what this module pooled.
    Nothing to do (and no library loaded) where no GPU test ran."""
    yield
    from broadway_amd import _lib
    if _lib._mi is not None:
        _lib._mi.h264mi_pool_drain()


# ------------------------------------------------------------------ CPU ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_generator_reproduces_fixture_streams(name):
    case_stream(name)
    if name in _golden.cases():        # the same stream as golden.json's case of that name
        assert _golden.cases()[name]["stream_sha256"] == CASES[name]["stream_sha256"]


def test_crop_offsets_zero_leave_streams_unchanged():
    a = gen.generate(2, 5, nframes=2, w_mbs=4, h_mbs=3, crop_bottom=4)
    assert a == gen.generate(2, 5, nframes=2, w_mbs=4, h_mbs=3, crop_bottom=4, crop_left=0, crop_top=0)
    assert a != gen.generate(2, 5, nframes=2, w_mbs=4, h_mbs=3, crop_bottom=4, crop_left=2)


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_testbench_reproduces_fixture(name):
    if not os.path.exists(_crop.REFDEC):
        pytest.skip("reference build not present")
    c = CASES[name]
    frames, crop, size = _crop.refdec_crop(case_stream(name))
    p = c["cropParams"]
    assert crop == (p["cropLeftOffset"], p["cropTopOffset"], p["cropOutWidth"], p["cropOutHeight"])
    assert size == (c["width"], c["height"]) and len(frames) == c["frames_total"]
    assert _golden.md5s(frames[:len(c["frames"])]) == c["frames"]


def test_reference_cropped_frames_are_numpy_crops_of_golden_frames():
    """crop.json and golden.json agree through the numpy restatement of
    CropPicture: cropping the oracle's full frames gives the cropped MD5s."""
    for name in ("crop_ltrb_6x4", "cfg1_plumbing_640x368"):
        c = CASES[name]
        p = c["cropParams"]
        frames, errs, w, h, _ = O.decode(case_stream(name))
        assert errs == 0 and (w, h) == (c["width"], c["height"])
        got = [_crop.crop_i420(f, w, h, p["cropLeftOffset"], p["cropTopOffset"], p["cropOutWidth"],
                               p["cropOutHeight"]).tobytes() for f in frames]
        assert _golden.md5s(got)[:len(c["frames"])] == c["frames"]


@pytest.fixture(scope="module")
def null_plain():
    """h264mi_dec on the CPU stand-in of the device (oracle/null_device.cpp),
    which has no crop entry points."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "nulldev-plain"], check=True)
    return os.path.join(ROOT, "oracle", "_build", "h264mi_dec_null_plain")


def test_null_backend_parses_crop_and_refuses_dash_C(null_plain, tmp_path):
    src = tmp_path / "in.h264"
    src.write_bytes(case_stream("crop_ltrb_6x4"))
    r = subprocess.run([null_plain, "-C", "-Onone", str(src)], capture_output=True, text=True)
    # the SPS through parse_sps and H264SwDecGetInfo, as the CLI prints it
    assert "Cropping params: (6, 2) 86x52" in r.stdout
    assert r.returncode != 0
    assert "not supported by this backend" in r.stderr
    # without -C the same build decodes the stream
    r = subprocess.run([null_plain, "-Onone", str(src)], capture_output=True, text=True)
    assert r.returncode == 0 and "pictures 5 errors 0" in r.stdout


# ------------------------------------------------------------------ GPU ----
def _mi():
    from broadway_amd import _lib
    return _lib.mi()


# (width, height, cpitch): a slot with padded chroma rows, and a packed one
PICS = {"48x32_pitch128": (48, 32, 128), "256x32_packed": (256, 32, 128)}
WINDOWS = [None, (2, 2, 2, 2), (6, 2, 38, 26), (0, 0, 46, 32), (44, 30, 4, 2)]


@pytest.fixture(scope="module")
def pictures():
    """name -> 3 random pictures in the (width, cpitch) layout (read-only)."""
    rng = np.random.default_rng(11)
    out = {}
    for name, (w, h, cp) in PICS.items():
        out[name] = [rng.integers(0, 256, w * h + cp * h, dtype=np.uint8) for _ in range(3)]
        for p in out[name]:
            p.setflags(write=False)
    return out


def expect(pic, w, h, cp, win, rgba):
    x, y, cw, ch = win
    i420 = _crop.crop_i420(pic, w, h, x, y, cw, ch, cpitch=cp)
    return np.frombuffer(O.yuv2rgba(i420.tobytes(), cw, ch), dtype=np.uint8) if rgba else i420


def run_crop(pics, w, h, cp, win, rgba, in_pad=0, out_pad=0, sentinel=0xA5):
    """h264mi_crop_device_pitch over `pics`; returns the whole output buffer
    (a sentinel-filled front pad of 64 bytes, then pictures out_stride apart)."""
    import torch
    L = _mi()
    x, y, cw, ch = win
    n = len(pics)
    nbytes = cw * ch * 4 if rgba else cw * ch * 3 // 2
    in_stride, out_stride = pics[0].size + in_pad, nbytes + out_pad
    host = np.zeros(in_stride * n, dtype=np.uint8)
    for k, p in enumerate(pics):
        host[k * in_stride:k * in_stride + p.size] = p
    d_in = torch.from_numpy(host).to("cuda")
    front = 64
    d_out = torch.full((front + out_stride * n + 64,), sentinel, dtype=torch.uint8, device="cuda")
    rc = L.h264mi_crop_device_pitch(d_in.data_ptr(), d_out.data_ptr() + front, w, h, cp, x, y, cw, ch, int(rgba), n,
                                    in_stride, out_stride, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy(), front, out_stride, nbytes


@pytest.mark.gpu
@pytest.mark.parametrize("rgba", [False, True], ids=["i420", "rgba"])
@pytest.mark.parametrize("pic", sorted(PICS))
def test_kernel_vs_numpy(pictures, pic, rgba):
    w, h, cp = PICS[pic]
    for win in WINDOWS + ([(252, 30, 4, 2), (130, 0, 126, 32)] if w == 256 else []):
        win = win or (0, 0, w, h)
        rc, out, front, stride, nbytes = run_crop(pictures[pic][:1], w, h, cp, win, rgba)
        assert rc == 0, win
        assert np.array_equal(out[front:front + nbytes], expect(pictures[pic][0], w, h, cp, win, rgba)), win
        assert (out[:front] == 0xA5).all() and (out[front + nbytes:] == 0xA5).all(), win


@pytest.mark.gpu
@pytest.mark.parametrize("rgba", [False, True], ids=["i420", "rgba"])
@pytest.mark.parametrize("pic", sorted(PICS))
def test_kernel_batched_padded_strides_write_nothing_else(pictures, pic, rgba):
    """npics = 3, padded strides: nothing before, between or after the
    pictures changes, the byte just past each picture included (a 16-byte
    tail overrun); the I420 strides make every picture start on another
    alignment."""
    w, h, cp = PICS[pic]
    # (RGBA output is 8-byte aligned: strides 8 and 0 mod 16, the 8- and 16-byte store forms)
    for win, out_pad in [(win, pad) for win in [(6, 2, 38, 26), (0, 0, w, h), (2, 2, 2, 2)]
                         for pad in ((40, 48) if rgba else (21,))]:
        rc, out, front, stride, nbytes = run_crop(pictures[pic], w, h, cp, win, rgba, in_pad=37, out_pad=out_pad)
        assert rc == 0, win
        assert (out[:front] == 0xA5).all(), win
        for k, p in enumerate(pictures[pic]):
            o = front + k * stride
            assert np.array_equal(out[o:o + nbytes], expect(p, w, h, cp, win, rgba)), (win, k)
            assert out[o + nbytes] == 0xA5, (win, k)
            assert (out[o + nbytes:o + stride] == 0xA5).all(), (win, k)
        assert (out[front + 3 * stride:] == 0xA5).all(), win


@pytest.mark.gpu
def test_kernel_full_window_packed_is_identity_and_yuv2rgba(pictures):
    import torch
    L = _mi()
    w, h, cp = PICS["256x32_packed"]
    p = pictures["256x32_packed"][0]
    rc, out, front, stride, nbytes = run_crop([p], w, h, cp, (0, 0, w, h), False)
    assert rc == 0 and np.array_equal(out[front:front + nbytes], p)
    rc, out, front, stride, nbytes = run_crop([p], w, h, cp, (0, 0, w, h), True)
    d_in = torch.from_numpy(np.array(p)).to("cuda")
    d_ref = torch.empty(w * h * 4, dtype=torch.uint8, device="cuda")
    assert L.h264mi_yuv2rgba_device(d_in.data_ptr(), d_ref.data_ptr(), w, h, 1, 0, 0,
                                    torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(out[front:front + nbytes], d_ref.cpu().numpy())


@pytest.mark.gpu
def test_kernel_rejects_bad_windows(pictures):
    w, h, cp = PICS["48x32_pitch128"]
    for win in [(1, 0, 2, 2), (0, 1, 2, 2), (0, 0, 3, 2), (0, 0, 2, 3), (0, 0, 50, 32), (46, 0, 4, 2),
                (0, 30, 2, 4), (-2, 0, 4, 4), (0, 0, 0, 2), (0, 0, 2, 0)]:
        for rgba in (False, True):
            rc, out, *_ = run_crop(pictures["48x32_pitch128"][:1], w, h, cp, win, rgba)
            assert rc == -1, win
            assert (out == 0xA5).all(), win          # nothing was launched


def decode_js(stream_nals, opts):
    got, dims = [], []
    dec = Decoder(opts)
    dec.onPictureDecoded = lambda buf, w, h, infos: (got.append(bytes(buf)), dims.append((w, h)))
    for nal in stream_nals:
        dec.decode(nal)
    info = dec.info()
    flag = int(info.croppingFlag)
    dec.close()
    return got, dims, flag


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_decoder_crop_option_vs_reference(name):
    c = CASES[name]
    p = c["cropParams"]
    nals = head_nals(case_stream(name), c)
    plain, pdims, _ = decode_js(nals, {})
    crop, cdims, flag = decode_js(nals, {"crop": True})
    rgb, rdims, _ = decode_js(nals, {"crop": True, "rgb": True})
    assert flag == 1
    assert len(crop) == len(rgb) == len(plain) == len(c["frames"])
    cw, ch = p["cropOutWidth"], p["cropOutHeight"]
    assert set(cdims) == set(rdims) == {(cw, ch)} and set(pdims) == {(c["width"], c["height"])}
    assert _golden.md5s(crop) == c["frames"]
    for f_crop, f_rgb in zip(crop, rgb):
        assert f_rgb == O.yuv2rgba(f_crop, cw, ch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_engine_read_crop_vs_numpy(name):
    """Engine.read_crop on reconstructed slots (one with padded chroma rows,
    one packed): both forms, the SPS window, against numpy on Engine.read."""
    from broadway_amd.engine import Capture, Engine
    c = CASES[name]
    p = c["cropParams"]
    win = (p["cropLeftOffset"], p["cropTopOffset"], p["cropOutWidth"], p["cropOutHeight"])
    cap = Capture(case_stream(name))
    eng = Engine(cap.w_mbs, cap.h_mbs, 1, cap.nslots)
    w, h = cap.w_mbs * 16, cap.h_mbs * 16
    for pic in cap.pictures:
        eng.decode([0], [pic])
        full = eng.read(0, pic.cur_slot)
        want = _crop.crop_i420(full, w, h, *win)
        assert np.array_equal(eng.read_crop(0, pic.cur_slot, *win), want)
        assert eng.read_crop(0, pic.cur_slot, *win, rgba=True).tobytes() == O.yuv2rgba(want.tobytes(), win[2], win[3])
    assert eng.errors() == 0
    with pytest.raises(RuntimeError):
        eng.read_crop(0, 0, 1, 0, 2, 2)


@pytest.mark.gpu
def test_switching_between_cropped_and_plain_output():
    """Once pictures leave cropped, the decoder stops queueing the uncropped
    copy behind each launch; a caller that goes back to NextPicture must
    still get every picture (read on demand)."""
    c = CASES["crop_ltrb_6x4"]
    full, _, w, h, _ = O.decode(case_stream("crop_ltrb_6x4"))
    got = []
    dec = Decoder({"crop": True})

    def on_picture(buf, pw, ph, infos):
        got.append((bytes(buf), pw, ph))
        dec._crop = len(got) in (1, 4)          # cropped: pictures 0, 1 and 4; plain: 2 and 3

    dec.onPictureDecoded = on_picture
    for nal in split_annexb(case_stream("crop_ltrb_6x4")):
        dec.decode(nal)
    dec.close()
    assert len(got) == len(full) == 5
    for k, (buf, pw, ph) in enumerate(got):
        if k in (0, 1, 4):
            assert (pw, ph) == (86, 52) and hashlib.md5(buf).hexdigest() == c["frames"][k], k
        else:
            assert (pw, ph) == (w, h) and buf == full[k], k


@pytest.mark.gpu
def test_no_crop_stream_is_byte_identical():
    c = _golden.cases()["small_ip_8x6_2sl"]
    nals = split_annexb(_golden.stream(c))
    plain, pdims, _ = decode_js(nals, {})
    crop, cdims, flag = decode_js(nals, {"crop": True})
    assert flag == 0 and plain == crop and pdims == cdims and len(plain) > 0
    rgb, _, _ = decode_js(nals, {"rgb": True})
    crgb, _, _ = decode_js(nals, {"crop": True, "rgb": True})
    assert rgb == crgb


@pytest.mark.gpu
def test_h264mi_dec_dash_C(tmp_path):
    exe = os.path.join(ROOT, "broadway_amd", "lib", "h264mi_dec")
    a, b = tmp_path / "a.h264", tmp_path / "b.h264"
    a.write_bytes(case_stream("crop_ltrb_6x4"))
    b.write_bytes(case_stream("crop_r_16x3"))
    c = CASES["crop_ltrb_6x4"]
    fb = 86 * 52 * 3 // 2
    for extra in (["-S2"], []):
        out = tmp_path / ("out%d.yuv" % len(extra))
        r = subprocess.run([exe, "-O" + str(out), "-C"] + extra + [str(a), str(b)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        assert "pictures 9 errors 0" in r.stdout and "Cropping params: (6, 2) 86x52" in r.stdout
        data = out.read_bytes()
        assert len(data) == fb * 5
        assert _golden.md5s([data[i:i + fb] for i in range(0, len(data), fb)]) == c["frames"]


NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "broadway_amd", "lib", "broadway.node")


@pytest.mark.gpu
@pytest.mark.skipif(not (NODE and os.path.exists(ADDON)), reason="node / addon not available")
def test_node_decoder_crop_option(tmp_path):
    """bindings/node: new Decoder({crop: true}) and {crop: true, rgb: true}."""
    c = CASES["crop_ltrb_6x4"]
    src = tmp_path / "s.h264"
    src.write_bytes(case_stream("crop_ltrb_6x4"))
    frames, _, w, h, _ = O.decode(case_stream("crop_ltrb_6x4"))
    want = [_crop.crop_i420(f, w, h, 6, 2, 86, 52).tobytes() for f in frames]
    for mode, exp, nbytes in (([], c["frames"], 86 * 52 * 3 // 2),
                              (["rgb"], _golden.md5s([O.yuv2rgba(f, 86, 52) for f in want]), 86 * 52 * 4)):
        r = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "decode_crop_md5.js"), str(src)] + mode,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out = json.loads(r.stdout.strip().splitlines()[-1])
        assert (out["width"], out["height"], out["bytes"]) == (86, 52, nbytes)
        assert out["frames"] == exp
