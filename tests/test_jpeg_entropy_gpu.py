"""The entropy decode on the device (include/ivit_jpeg_entropy.h): ivit_jpeg_entropy_decode against the host decoder's coefficients,
every one, over the accepted files of tests/golden/jpeg.npz and the files of tests/golden/jpeg_entropy.npz, in one ragged batch and
alone, at the smallest and at the default subsequence; the refusals behind the headers between two good files; guards around every
array; `jpeg.decode(..., entropy="device")` against the host path; the entry captured and replayed.  The reference is the host decoder
(and Pillow's recorded bytes behind the reconstruction), never the code under test."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from ivit_amd import _lib  # noqa: E402
from ivit_amd import jpeg as J  # noqa: E402

GUARD, FILL = 4096, 0xA5
FIXTURE = [str(n) for n in load_golden("jpeg_entropy.npz")["names"]]


@functools.lru_cache(None)
def files():
    g, e = load_golden("jpeg.npz"), load_golden("jpeg_entropy.npz")
    out = {str(n): g["jpg_" + str(n)].tobytes() for n in list(g["accepted"]) + list(g["refused"])}
    out.update((n, e["jpg_" + n].tobytes()) for n in FIXTURE)
    return out


def accepted():
    return [str(n) for n in load_golden("jpeg.npz")["accepted"]] + FIXTURE


@functools.lru_cache(None)
def host(name):
    """the reference: the host decoder's coefficients of a file"""
    return J.entropy_decode(files()[name])[1]


def _guarded(a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([np.full(GUARD, FILL, np.uint8), a, np.full(GUARD, FILL, np.uint8)])).cuda()


class Batch:
    """B files in guarded device arrays; `room`: bytes of the stream and workspace buffers beyond what the files need"""
    def __init__(self, datas, room=0):
        sc = [J.scan(d) for d in datas]
        self.B = len(sc)
        self.table, self.nc, self.npx, self.nws = J.layout([s[0] for s in sc], [s[4] for s in sc], [s[5] for s in sc])
        self.stable, self.segs, nstream, wsb = J.entropy_layout([s[1] for s in sc], [s[3] for s in sc])
        streams = np.zeros(nstream + room, np.uint8)
        for k, s in enumerate(sc):
            streams[self.stable[k].stream_offset:][:len(s[2])] = s[2]
        self.streams, self.segs_dev = _guarded(streams), _guarded(self.segs)
        self.desc_dev = _guarded(np.frombuffer(self.table, np.uint8, self.B * ctypes.sizeof(_lib.JpegDesc)))
        self.scan_dev = _guarded(np.frombuffer(self.stable, np.uint8, self.B * ctypes.sizeof(_lib.JpegScan)))
        self.inputs = [t.clone() for t in (self.streams, self.segs_dev, self.desc_dev, self.scan_dev)]
        self.work, self.coefs, self.status = (_guarded(np.full(n, FILL, np.uint8)) for n in (wsb + room, 2 * self.nc, 4 * self.B))

    def view(self, t, dtype=torch.uint8):
        return t[GUARD:t.numel() - GUARD].view(dtype)

    def call(self, h, bits):
        J.entropy_decode_device(self.view(self.streams), self.table, self.view(self.desc_dev), self.stable, self.view(self.scan_dev), self.segs,
                                self.view(self.segs_dev), self.B, self.view(self.work), self.view(self.coefs, torch.int16),
                                self.view(self.status, torch.int32), bits, h=h)

    def results(self):
        """checks the guards and the inputs -> (coefficients per file, status)"""
        torch.cuda.synchronize()
        for t in (self.work, self.coefs, self.status):
            assert (t[:GUARD] == FILL).all().item() and (t[-GUARD:] == FILL).all().item(), "wrote outside an output"
        for t, was in zip((self.streams, self.segs_dev, self.desc_dev, self.scan_dev), self.inputs):
            assert torch.equal(t, was), "an input changed"
        c = self.view(self.coefs, torch.int16).cpu().numpy()
        return [c[d.coef_offset:][:64 * sum(b * h for b, h in zip(d.bw, d.bh))] for d in self.table[:self.B]], self.view(self.status, torch.int32).cpu().numpy()


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("bits", [_lib.IVIT_JPEG_ENTROPY_MIN_BITS, 0], ids=["smallest", "default"])
@pytest.mark.parametrize("which", ["all"] + FIXTURE)
def test_coefficients_are_the_host_decoders(H, which, bits):
    names = accepted() if which == "all" else [which]
    b = Batch([files()[n] for n in names])
    b.call(H, bits)
    coefs, status = b.results()
    assert not status.any(), [(n, s) for n, s in zip(names, status) if s]
    for n, c in zip(names, coefs):
        assert np.array_equal(c, host(n)), (n, int((c != host(n)).sum()))
    if which == "all":                                        # ... and the reconstruction of them is Pillow's bytes
        g = load_golden("jpeg.npz")
        pixels, work = torch.zeros(b.npx, dtype=torch.uint8, device="cuda"), torch.zeros(b.nws, dtype=torch.uint8, device="cuda")
        J.reconstruct(b.view(b.coefs, torch.int16), b.table, b.B, pixels, work, table_dev=b.view(b.desc_dev), h=H)
        px = pixels.cpu().numpy()
        for n, d in zip(names, b.table):
            if "rgb_" + n in g.files:
                assert np.array_equal(px[d.pixel_offset:][:g["rgb_" + n].size], g["rgb_" + n].reshape(-1)), n


@pytest.mark.parametrize("name", ["trunc_691", "trunc_728", "trunc_729", "trunc_730", "dqt255"])
def test_refusal_between_two_good_files(H, name):
    """the refused files whose refusal lies behind the headers.  The truncations end without EOI, which the pre-pass refuses with the
    host decoder's status; given the EOI it asks for, their data reaches the device, which must reach the host decoder's verdict on
    those bytes: the data ends before the last MCU, or, where only the EOI was cut, nothing is wrong"""
    g = load_golden("jpeg.npz")
    want = int(g["refused_status"][list(g["refused"]).index(name)])
    data = files()[name]
    try:
        J.scan(data)
    except J.JpegRefused as e:
        assert e.status == want
        data += b"\xff\xd9"
    try:
        middle, want = J.entropy_decode(data)[1], _lib.IVIT_OK
    except J.JpegRefused as e:
        assert e.status == want
        middle = None
    good = ["53x37_noise_q85_s2", "rst1_grey"]
    b = Batch([files()[good[0]], data, files()[good[1]]])
    b.call(H, 0)
    coefs, status = b.results()
    assert status[0] == 0 == status[2] and J.status_class(int(status[1])) == want, status
    assert np.array_equal(coefs[0], host(good[0])) and np.array_equal(coefs[2], host(good[1]))
    assert middle is None or np.array_equal(coefs[1], middle)


def test_decode_with_device_entropy_equals_the_host_path():
    pytest.importorskip("PIL")
    names = ["16x16_noise_q85_s2", "progressive", "grad_q30_s2_rst1", "7x9_grad_q30_grey", "cmyk", "dqt255", "rst1_s0", "grey_q85",
             "restart_out_of_sequence", "1x1_noise_q85_s0"]
    datas = [files()[n] for n in names]
    a, fa = J.decode(datas, "cuda", threads=3)
    b, fb = J.decode(datas, "cuda", threads=3, entropy="device")
    assert fa == fb and [i for i, _ in fb] == [1, 4, 5, 8]
    assert np.array_equal(a.desc, b.desc) and torch.equal(a.pixels, b.pixels)
    with pytest.raises(J.JpegRefused) as e:
        J.decode([datas[0], files()["trunc_691"]], "cuda", fallback="raise", entropy="device")
    assert e.value.status == _lib.IVIT_ERR_INVALID


def test_captured_entry_replays_over_new_streams():
    """captured on a side stream, nothing runs before the launch; the replay gives the eager bytes, and — the kernel reads only the
    device copies — the host decoder's coefficients of another file of the same geometry once its stream and tables lie there"""
    first, second = Batch([files()["53x37_noise_q85_s2"]], room=4096), Batch([files()["opt_s2"]], room=4096)
    assert bytes(first.table[0])[:72] == bytes(second.table[0])[:72] and len(first.segs) == len(second.segs) == 1
    stream = torch.cuda.Stream()
    h = _lib.Handle(0, stream.cuda_stream)
    with torch.cuda.stream(stream):                          # eager once: the code is loaded outside the capture
        first.call(h, 0)
    eager, status = first.results()
    assert status[0] == 0 and np.array_equal(eager[0], host("53x37_noise_q85_s2"))
    first.view(first.coefs).fill_(FILL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
        first.call(h, 0)
    torch.cuda.synchronize()
    assert (first.coefs == FILL).all().item()                # captured, not run
    for _ in range(3):
        first.view(first.coefs).fill_(FILL)
        torch.cuda.synchronize()
        graph.replay()
        coefs, status = first.results()
        assert status[0] == 0 and np.array_equal(coefs[0], eager[0])
    for mine, other in ((first.streams, second.streams), (first.segs_dev, second.segs_dev), (first.desc_dev, second.desc_dev),
                        (first.scan_dev, second.scan_dev)):
        n = min(mine.numel(), other.numel()) - 2 * GUARD
        first.view(mine)[:n] = second.view(other)[:n]
    first.inputs = [t.clone() for t in (first.streams, first.segs_dev, first.desc_dev, first.scan_dev)]
    graph.replay()
    coefs, status = first.results()
    assert status[0] == 0 and np.array_equal(coefs[0], host("opt_s2")) and not np.array_equal(coefs[0], eager[0])
