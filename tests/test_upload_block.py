"""lld_upload_block.h on the CPU: the block builder that lays out, stages and binds the arrays of a tracking-stage upload.  The header is
compiled without HIP into a stand-alone C++17 program (-Wall -Werror; with gcc's address and undefined-behaviour sanitizers linked
statically when their runtimes are installed).  The program declares one block of every element size the chain uses at every count below,
stages each array from a source or from a fill byte over a canary, and prints what it laid out and what it found; the offsets are compared
with the layout rule restated here.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [0, 1, 63, 64, 65, 256, 257]       # 256 / 257 one-byte elements: an array of exactly 256 bytes and one of 257
# (C++ element type, elements per entry): bytes, 4-byte words, doubles, float[3], double[3], 32-byte descriptors
TYPES = [("uint8_t", 1, 1), ("int32_t", 1, 4), ("double", 1, 8), ("float", 3, 12), ("double", 3, 24), ("uint32_t", 8, 32)]
FILLS = [0x01, 0x00, 0xFF]                  # has_obs, skip / kp_outlier, ln_line_id
CANARY = 0xA5


def arrays():
    """(type, per, element bytes, count, fill or None = staged from a source) in declaration order; every size meets every way of staging."""
    out = []
    for ti, (t, per, eb) in enumerate(TYPES):
        for ci, n in enumerate(COUNTS):
            k = ti + ci
            out.append((t, per, eb, n, None if k % 2 == 0 else FILLS[(k // 2) % 3]))
    return out


UPLOADED = 3 * len(COUNTS)                  # the arrays declared before end_upload(); a zero-count array sits right at the boundary


SOURCE = r"""
#include <cstdio>
#include <vector>
#include "%(root)s/lld_slam_amd/csrc/lld_upload_block.h"

using namespace lld_track;

struct Rec { size_t off, bytes; int fill; int id; bool ptrs; };
static std::vector<Rec> recs;
static unsigned char src_byte(int id, size_t j) { return (unsigned char)(id * 31 + j * 7 + 1); }

template <class T>
static void add(UploadBlock& B, size_t n, size_t per, int fill) {
  const int id = (int)recs.size();
  const Span<T> s = B.take<T>(n, per);
  const size_t bytes = n * per * sizeof(T);
  std::vector<unsigned char> raw(bytes + sizeof(T));
  for (size_t j = 0; j < bytes; j++) raw[j] = src_byte(id, j);
  std::vector<T> src(n * per + 1);
  std::memcpy(src.data(), raw.data(), bytes);
  B.stage(s, fill < 0 ? src.data() : static_cast<const T*>(nullptr), fill < 0 ? 0 : fill);
  const bool ptrs = reinterpret_cast<char*>(B.host(s)) == B.h + s.off && reinterpret_cast<char*>(B.dev(s)) == B.d + s.off && s.n == n * per;
  recs.push_back(Rec{s.off, bytes, fill, id, ptrs});
}

int main() {
  const size_t cap = %(cap)d;
  unsigned char* host = new unsigned char[cap];
  std::memset(host, %(canary)d, cap);
  char* const dev = reinterpret_cast<char*>(uintptr_t(1) << 40);        // never dereferenced
  UploadBlock B;
  B.bind(reinterpret_cast<char*>(host), dev);
%(adds)s
  if (B.size + 256 > cap) { std::printf("capacity\n"); return 1; }
  for (size_t a = 0; a < recs.size(); a++) {
    const Rec& r = recs[a];
    const size_t next = a + 1 < recs.size() ? recs[a + 1].off : B.size;
    size_t bad = 0, spilled = 0;
    for (size_t j = 0; j < r.bytes; j++) bad += host[r.off + j] != (r.fill < 0 ? src_byte(r.id, j) : (unsigned char)r.fill);
    for (size_t j = r.off + r.bytes; j < next + (a + 1 == recs.size() ? 256 : 0); j++) spilled += host[j] != %(canary)d;   // padding, and past the block's end
    const int after = host[r.off + r.bytes];      // the byte behind the array: canary, or the first byte of the neighbour that starts there
    std::printf("%%zu %%zu %%zu %%zu %%d %%d\n", r.off, r.bytes, bad, spilled, after, (int)r.ptrs);
  }
  std::printf("%%zu %%zu\n", B.up_bytes, B.size);
  delete[] host;
  return 0;
}
"""


def have_static_sanitizers():
    def found(name):
        return os.path.isabs(subprocess.check_output(["g++", "-print-file-name=" + name], text=True).strip())
    return found("libasan.a") and found("libubsan.a")


def al(b):
    return (b + 255) & ~255


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("upload_block")
    adds = []
    for i, (t, per, _, n, fill) in enumerate(arrays()):
        if i == UPLOADED:
            adds.append("  B.end_upload();")
        adds.append("  add<%s>(B, %d, %d, %d);" % (t, n, per, -1 if fill is None else fill))
    cap = sum(al(n * eb) for _, _, eb, n, _ in arrays()) + 256
    src = d / "block.cpp"
    src.write_text(SOURCE % dict(root=ROOT, cap=cap, canary=CANARY, adds="\n".join(adds)))
    exe = d / "block"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + (san if have_static_sanitizers() else []) +
                          [str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert len(out) == len(arrays()) + 1
    return [[int(x) for x in ln.split()] for ln in out]


def test_the_cases_cover_the_sizes():
    A = arrays()
    assert {eb for _, _, eb, _, _ in A} == {1, 4, 8, 12, 24, 32}
    for eb in (1, 4, 8, 12, 24, 32):
        assert {0, 1, 63, 64, 65} <= {n for _, _, e, n, _ in A if e == eb}
    assert {256, 257} <= {n * eb for _, _, eb, n, _ in A}
    for eb in (1, 4, 8, 12, 24, 32):                                   # every element size is staged both ways, and filled with every byte somewhere
        assert {f is None for _, _, e, n, f in A if e == eb and n} == {True, False}
    assert {f for _, _, _, n, f in A if n and f is not None} == set(FILLS)
    assert A[UPLOADED][3] == 0                                          # a zero-count array is the first one behind the boundary


def test_layout_is_aligned_disjoint_and_in_declaration_order(lines):
    A = arrays()
    at = 0
    for (off, nbytes, _, _, _, _), (_, _, eb, n, _) in zip(lines[:-1], A):
        assert off % 256 == 0
        assert off == at and nbytes == n * eb                           # an array starts where its predecessor's padded extent ends
        at += al(n * eb)
    offs = [ln[0] for ln in lines[:-1]]
    assert offs == sorted(offs)
    for (off, nbytes, *_), nxt in zip(lines[:-1], offs[1:] + [at]):
        assert off + nbytes <= nxt                                      # disjoint
    up_bytes, size = lines[-1]
    assert size == at
    assert up_bytes == offs[UPLOADED] == sum(al(n * eb) for _, _, eb, n, _ in A[:UPLOADED])


def test_a_count_of_zero_takes_no_bytes(lines):
    A = arrays()
    zeros = [i for i, a in enumerate(A) if a[3] == 0]
    assert len(zeros) == len(TYPES)
    offs = [ln[0] for ln in lines[:-1]] + [lines[-1][1]]
    for i in zeros:
        assert lines[i][1] == 0 and offs[i + 1] == offs[i]
        if i > 0:
            assert lines[i - 1][2] == 0 and lines[i - 1][3] == 0        # its neighbours hold what was staged into them
        if i + 1 < len(A):
            assert lines[i + 1][2] == 0


def test_staged_bytes_and_fill_bytes_cover_exactly_the_array(lines):
    A = arrays()
    for i, ((off, nbytes, bad, spilled, after, _), (_, _, _, _, fill)) in enumerate(zip(lines[:-1], A)):
        assert bad == 0, "array %d: %d bytes differ from the %s" % (i, bad, "source" if fill is None else "fill byte")
        assert spilled == 0, "array %d: %d bytes of padding behind it were written" % (i, spilled)
        if nbytes % 256:
            assert after == CANARY                                      # the byte behind the array is untouched padding


def test_typed_pointers_are_base_plus_offset(lines):
    assert all(ln[5] == 1 for ln in lines[:-1])
