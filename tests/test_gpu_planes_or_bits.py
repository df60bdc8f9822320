"""-m gpu: the reduction that proves the planar contract (kernels_reduce.hip: k_planes_or_bits, through the C entry
t8gpu_hip_planes_or_bits_{f32,f64}) against np.bitwise_or.reduce over the words of each plane. Every comparison is exact.

If the kernel misses one set bit, the native stepper runs the planar 2D stage on a state that has a z-momentum. Its paths: the
words before the first 16-byte boundary (head), 16-byte vectors in a four-deep unrolled grid-stride loop, a one-vector remainder
loop, fewer than four words behind the last vector (tail), at most 2048 workgroups per plane, one atomic OR per workgroup.

Layout of every case: the four planes lie in one buffer whose other words are all ones -- eight words of them before and at least
eight behind each plane -- so that a read outside a plane shows as set bits; each plane starts at its own offset from a 16-byte
boundary (fp32: 0 .. 3 words; fp64: 0 or 1 element = 0 or 2 words)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _scalar_ref as R
from t8gpu_amd import hip

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
GUARD = 8                                  # words of all ones before and behind each plane (a multiple of 4: keeps the alignment)
ONES = np.uint32(0xFFFFFFFF)
BITS = (np.uint32(1), np.uint32(0x80000000))   # bit 0: a denormal's low word; bit 31: the sign (-0.0f, the high word of a -0.0 double)
INVALID = 1                                # hipErrorInvalidValue


def entry(dtype):
    fn = getattr(hip.lib(), f"t8gpu_hip_planes_or_bits_{hip.suffix(dtype)}")
    fn.restype = C.c_int
    fn.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def offsets(dtype, rot):
    """word offsets of the four planes from a 16-byte boundary: all different in fp32, both possible ones in fp64"""
    return [(j + rot) % 4 if dtype == torch.float32 else 2 * ((j + rot) % 2) for j in range(4)]


class Planes:
    """four zeroed planes of `n` elements inside a buffer of ones; a host mirror receives every write the device buffer does"""

    def __init__(self, dtype, n, rot=0):
        self.dtype, self.n = dtype, n
        self.nwords = n * (2 if dtype == torch.float64 else 1)
        self.off = offsets(dtype, rot)
        span = GUARD + 4 + ((self.nwords + 3) // 4) * 4 + GUARD          # a multiple of 4 words per plane
        self.start = [j * span + GUARD + self.off[j] for j in range(4)]
        self.host = np.full(4 * span, ONES, np.uint32)
        self.dev = torch.full((4 * span,), -1, dtype=torch.int32, device="cuda")
        for s in self.start:
            self.host[s:s + self.nwords] = 0
            self.dev[s:s + self.nwords].zero_()
        assert self.dev.data_ptr() % 16 == 0
        self.ptrs = (C.c_void_p * 4)(*[self.dev.data_ptr() + 4 * s for s in self.start])
        self.head = [min((4 - o) % 4, self.nwords) for o in self.off]    # words before the first 16-byte boundary
        self.fn = entry(dtype)

    def put(self, plane, word, value):
        """one word of one plane, on the host mirror and (stream-ordered) on the device"""
        assert 0 <= word < self.nwords
        i = self.start[plane] + word
        self.host[i] = value
        self.dev[i] = int(np.uint32(value).view(np.int32))

    def launch(self, out):
        """out: int32 device tensor of 4 words"""
        code = self.fn(self.n, C.cast(self.ptrs, C.c_void_p), C.c_void_p(out.data_ptr()), hip.stream_ptr())
        assert code == 0, code

    def want(self):
        """the reference: np.bitwise_or.reduce over the words of each plane, from the host mirror"""
        return [R.or_bits(self.host[s:], self.nwords) for s in self.start]

    def run_single_bits(self, cases):
        """cases: (plane, word, bit). One launch per case with exactly that bit set, each into a row of its own of a zeroed
        result array (read back once); returns (got [len(cases), 4], want [len(cases), 4])"""
        outs = torch.zeros((len(cases), 4), dtype=torch.int32, device="cuda")
        want = np.zeros((len(cases), 4), np.uint32)
        for k, (plane, word, bit) in enumerate(cases):
            self.put(plane, word, bit)
            self.launch(outs[k])
            want[k] = self.want()
            assert want[k, plane] == bit and want[k].sum() == bit
            self.put(plane, word, 0)
        torch.cuda.synchronize()
        return outs.cpu().numpy().view(np.uint32), want


def assert_exact(got, want, cases):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(cases[k], got[k].tolist(), want[k].tolist()) for k in bad[:5]]


SMALL = [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", SMALL)
def test_small_sizes(dtype, n):
    """n <= 1025: every word position of a plane with bit 0 and with bit 31, the plane that holds the bit rotating with the
    position; above, the first and last 12 words and 64 random positions. All-zero planes give 0 although their surroundings
    are all ones."""
    P = Planes(dtype, n, rot=n % 4)
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    P.launch(out)
    assert out.tolist() == [0, 0, 0, 0] == P.want()
    nw = P.nwords
    if n <= 1025:
        words = range(nw)
    else:
        rng = np.random.default_rng(n)
        words = sorted(set(range(12)) | set(range(nw - 12, nw)) | set(rng.integers(0, nw, 64).tolist()))
    cases = [((w + b) % 4, w, BITS[b]) for w in words for b in (0, 1)]
    got, want = P.run_single_bits(cases)
    assert_exact(got, want, cases)


@pytest.mark.parametrize("dtype,n", [(torch.float32, 100003), (torch.float64, 50001)], ids=IDS)
@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_medium_size(dtype, n, rot):
    """100 003 words per plane (fp64: 50 001 elements = 100 002 words, the number of words of a double plane is even), 25
    workgroups, the unrolled loop and the remainder loop both run. Per plane, from its own head: the first and the last word,
    the last head word, each word of the first and of the last body vector, every tail word, 64 random positions."""
    P = Planes(dtype, n, rot)
    nw = P.nwords
    rng = np.random.default_rng(100 + rot)
    cases = []
    for plane in range(4):
        head = P.head[plane]
        nvec = (nw - head) // 4
        tail = nw - head - 4 * nvec
        assert nvec > 3 * 25 * 256 + 256                       # (some lanes take the unrolled round, the others the remainder loop)
        words = {0, nw - 1} | set(range(head, head + 4)) | set(range(head + 4 * (nvec - 1), head + 4 * nvec))
        words |= set(range(nw - tail, nw)) | set(rng.integers(0, nw, 64).tolist())
        if head:
            words.add(head - 1)
        cases += [(plane, w, BITS[(w + k) % 2]) for k, w in enumerate(sorted(words))]
    got, want = P.run_single_bits(cases)
    assert_exact(got, want, cases)
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    P.launch(out)
    assert out.tolist() == [0, 0, 0, 0]


# Past the block cap: 2048 workgroups x 4096 words is what one round of the unrolled loop covers, so
#   fp32: n = 8 388 613 elements = 2048 * 4096 + 5 words;   fp64: n = 4 194 307 elements = 8 388 614 words = 2048 * 4096 + 6.
# The kernel's `step` is gridDim.x * 256 = 524 288 vectors. Lane t of workgroup b starts at vector i = 256 b + t < step and loads
# v[i], v[i + step], v[i + 2 step], v[i + 3 step] in its one unrolled round (i + 3 step < nvec holds for every lane): quarter q of
# the range is load q. Then i += 4 step = 2 097 152, and only where nvec > 4 step (a head of 0 or 1 word in fp32, of 0 in fp64)
# one vector is left for the remainder loop: vector 4 step, taken by lane 0 of workgroup 0.
BIG = {torch.float32: 8388613, torch.float64: 4194307}
STEP = 2048 * 256


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_past_the_block_cap(dtype):
    P = Planes(dtype, BIG[dtype], rot=0)
    nw = P.nwords
    assert nw > 2048 * 4096 and (nw + 4095) // 4096 > 2048
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    P.launch(out)
    assert out.tolist() == [0, 0, 0, 0] == P.want()
    plane = 0                                                   # offset 0: head 0, so nvec = nw // 4 = 4 step + 1
    head, nvec = P.head[plane], (nw - P.head[plane]) // 4
    assert head == 0 and nvec == 4 * STEP + 1
    cases = [(plane, 0, BITS[1]), (plane, nw - 1, BITS[0])]
    for q in range(4):                                          # load q of the unrolled round, a lane in the middle of the grid
        vec = q * STEP + 256 * (511 * (q + 1)) + 37 * (q + 1)
        assert q * STEP <= vec < (q + 1) * STEP
        cases.append((plane, head + 4 * vec + q, BITS[q % 2]))
    cases.append((plane, head + 4 * (4 * STEP) + 2, BITS[1]))   # the remainder loop's only vector
    other = 3                                                   # fp32: offset 3, head 1; fp64: offset 2, head 2: its last vector
    h3 = P.head[other]
    cases.append((other, h3 + 4 * ((nw - h3) // 4 - 1) + 3, BITS[0]))
    got, want = P.run_single_bits(cases)
    assert_exact(got, want, cases)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_accumulates_into_out(dtype):
    """out4[j] |= ...: the stepper clears out4 before the call; the kernel itself only ORs into it"""
    P = Planes(dtype, 1000, rot=1)
    P.put(1, 3, 0x00000F00)
    P.put(2, P.nwords - 1, 0x80000000)
    pattern = np.array([0x0000A5A5, 0x00000033, 0x00000001, 0x7FFFFFFF], np.uint32)
    out = torch.from_numpy(pattern.view(np.int32).copy()).cuda()
    P.launch(out)
    assert out.cpu().numpy().view(np.uint32).tolist() == (pattern | np.array(P.want(), np.uint32)).tolist()
    assert P.want() == [0, 0x00000F00, 0x80000000, 0]
    P.launch(out)                                               # and again: nothing changes
    assert out.cpu().numpy().view(np.uint32).tolist() == (pattern | np.array(P.want(), np.uint32)).tolist()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_bit_of_a_word(dtype):
    """a word of all ones, and two words whose bits only together cover a pattern"""
    P = Planes(dtype, 257, rot=2)
    P.put(0, 0, 0xFFFFFFFF)
    P.put(1, 5, 0x0F0F0000)
    P.put(1, P.nwords - 1, 0x00000F0F)
    P.put(3, P.nwords // 2, 0x12345678)
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    P.launch(out)
    assert out.cpu().numpy().view(np.uint32).tolist() == [0xFFFFFFFF, 0x0F0F0F0F, 0, 0x12345678] == P.want()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_and_refused_calls(dtype):
    P = Planes(dtype, 16)
    fn = P.fn
    pattern = [0x5A5A5A5A, 1, 0, 0x7FFFFFFF]
    out = torch.tensor(pattern, dtype=torch.int32, device="cuda")
    P.put(0, 0, 0xFFFFFFFF)
    planes, stream = C.cast(P.ptrs, C.c_void_p), hip.stream_ptr()
    assert fn(0, planes, C.c_void_p(out.data_ptr()), stream) == 0                     # n == 0: nothing to do, out untouched
    torch.cuda.synchronize()
    assert out.tolist() == pattern
    assert fn(16, planes, None, stream) == INVALID                                   # a null out
    assert fn(16, None, C.c_void_p(out.data_ptr()), stream) == INVALID               # a null array of planes
    for j in range(4):                                                               # a null plane
        ptrs = (C.c_void_p * 4)(*[None if k == j else P.ptrs[k] for k in range(4)])
        assert fn(16, C.cast(ptrs, C.c_void_p), C.c_void_p(out.data_ptr()), stream) == INVALID
    torch.cuda.synchronize()
    assert out.tolist() == pattern                                                   # no refused call wrote anything
