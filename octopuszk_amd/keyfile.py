"""The Groth16 proving-key file (OZKPK version 1): layout, writer and strict parser.  Host
only: nothing here touches the GPU; zksnark.py decodes the points it reads from here on the device.

All integers little-endian.  Points in the compressed encoding of section 13 (G1 32 bytes, G2 64).

    header   8   magic and version  OZKPK\\0\\0\\1
             16  num_inputs, num_auxiliary, num_constraints, m (the domain size)   4 x u32
             32  SHA-256 of every byte after the header
             13 x 20  section table: (u32 id, u64 offset from the start of the file, u64 byte length), ids 1 .. 13
    sections alpha_g1, beta_g1, delta_g1 (32 each), beta_g2, delta_g2 (64 each), query_a (nv x 32), query_b_g1
             (nv x 32), query_b_g2 (nv x 64), delta_abc_g1 ((nv - ni) x 32), query_h ((m + 1) x 32), r1cs_a, r1cs_b,
             r1cs_c
    r1cs_*   u32 rows, u32 nnz, u32 has_values, (rows + 1) x u32 row offsets, nnz x u32 variable indices,
             has_values ? nnz x 32-byte coefficients : nothing  — the R1CSRelation as given

Every point array has a fixed stride, so rows [lo, hi) of one are the bytes [offset + lo * stride, offset + hi * stride)
and a rank of a sharded prover reads its slices and nothing else.  The parser raises ValueError naming what is wrong.
"""
import hashlib
import struct

import numpy as np

MAGIC = b"OZKPK\x00\x00\x01"
FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
# (name, bytes per row or None for an R1CS section, row count as a function of the header)
SECTIONS = (
    ("alpha_g1", 32, lambda h: 1), ("beta_g1", 32, lambda h: 1), ("delta_g1", 32, lambda h: 1),
    ("beta_g2", 64, lambda h: 1), ("delta_g2", 64, lambda h: 1),
    ("query_a", 32, lambda h: h.nv), ("query_b_g1", 32, lambda h: h.nv), ("query_b_g2", 64, lambda h: h.nv),
    ("delta_abc_g1", 32, lambda h: h.nv - h.num_inputs), ("query_h", 32, lambda h: h.m + 1),
    ("r1cs_a", None, None), ("r1cs_b", None, None), ("r1cs_c", None, None))
NAMES = tuple(s[0] for s in SECTIONS)
STRIDE = {name: stride for name, stride, _ in SECTIONS if stride}
HEADER_BYTES = 8 + 16 + 32 + 20 * len(SECTIONS)
_ENTRY = struct.Struct("<IQQ")


def _domain(nc, ni):
    m = 1
    while m < nc + ni:
        m *= 2
    return m


# ---------------------------------------------------------------------------- R1CS sections
def r1cs_section(ptr, index, value=None) -> bytes:
    """One side (A, B or C) of an R1CSRelation: row offsets, variable indices, coefficients or None (all one)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    index = np.asarray(index, dtype=np.int64)
    rows, nnz = len(ptr) - 1, len(index)
    out = [struct.pack("<III", rows, nnz, 0 if value is None else 1), ptr.astype("<u4").tobytes(),
           index.astype("<u4").tobytes()]
    if value is not None:
        if len(value) != nnz:
            raise ValueError("%d coefficients for %d terms" % (len(value), nnz))
        out.append(b"".join(int(v).to_bytes(32, "little") for v in value))
    return b"".join(out)


def _below_r(raw, nnz):
    """per 32-byte little-endian value of raw: value < r"""
    v = np.frombuffer(raw, dtype=np.uint8).reshape(nnz, 32)[:, ::-1].astype(np.int16)
    d = v - np.frombuffer(FR.to_bytes(32, "big"), dtype=np.uint8).astype(np.int16)
    nz = d != 0
    first = nz.argmax(axis=1)
    return nz.any(axis=1) & (d[np.arange(nnz), first] < 0)


def parse_r1cs_section(name, b, rows_expected, nv):
    """(row offsets int64, indices int64, coefficients as an object array of ints or None)"""
    if len(b) < 12:
        raise ValueError("section %s: %d bytes do not hold its three counts" % (name, len(b)))
    rows, nnz, has_values = struct.unpack_from("<III", b, 0)
    if has_values > 1:
        raise ValueError("section %s: has_values is %d" % (name, has_values))
    if rows != rows_expected:
        raise ValueError("section %s: %d rows, the header says %d constraints" % (name, rows, rows_expected))
    want = 12 + 4 * (rows + 1) + 4 * nnz + 32 * nnz * has_values
    if len(b) != want:
        raise ValueError("section %s: %d bytes, its counts say %d" % (name, len(b), want))
    ptr = np.frombuffer(b, dtype="<u4", count=rows + 1, offset=12).astype(np.int64)
    idx = np.frombuffer(b, dtype="<u4", count=nnz, offset=12 + 4 * (rows + 1)).astype(np.int64)
    if ptr[0] != 0 or (np.diff(ptr) < 0).any():
        raise ValueError("section %s: row offsets are not non-decreasing from 0" % name)
    if ptr[-1] != nnz:
        raise ValueError("section %s: row offsets end at %d, not at nnz = %d" % (name, int(ptr[-1]), nnz))
    if nnz and idx.max() >= nv:
        bad = int((idx >= nv).argmax())
        raise ValueError("section %s: term %d has variable index %d >= %d" % (name, bad, int(idx[bad]), nv))
    value = None
    if has_values:
        raw = b[12 + 4 * (rows + 1) + 4 * nnz:]
        ok = _below_r(raw, nnz) if nnz else np.ones(0, dtype=bool)
        if not ok.all():
            raise ValueError("section %s: coefficient %d is >= r" % (name, int((~ok).argmax())))
        value = np.array([int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(nnz)], dtype=object)
    return ptr, idx, value


# ---------------------------------------------------------------------------- writer
def build(num_inputs, num_auxiliary, num_constraints, sections) -> bytes:
    """The file of a key: `sections` maps every name of NAMES to its bytes (compressed points, r1cs_section)."""
    h = Header(num_inputs, num_auxiliary, num_constraints, _domain(num_constraints, num_inputs), None, None)
    table, off = [], HEADER_BYTES
    for i, (name, stride, count) in enumerate(SECTIONS):
        b = sections[name]
        if stride and len(b) != stride * count(h):
            raise ValueError("section %s: %d bytes, the counts say %d" % (name, len(b), stride * count(h)))
        table.append(_ENTRY.pack(i + 1, off, len(b)))
        off += len(b)
    payload = b"".join(bytes(sections[name]) for name in NAMES)
    return b"".join([MAGIC, struct.pack("<IIII", num_inputs, num_auxiliary, num_constraints, h.m),
                     hashlib.sha256(payload).digest()] + table + [payload])


# ---------------------------------------------------------------------------- parser
class Header:
    def __init__(self, num_inputs, num_auxiliary, num_constraints, m, digest, table):
        self.num_inputs, self.num_auxiliary, self.num_constraints, self.m = num_inputs, num_auxiliary, num_constraints, m
        self.nv = num_inputs + num_auxiliary
        self.digest, self.table = digest, table   # table: name -> (offset, length)


class _Bytes:
    """bytes behind the seek / read / tell of a file"""

    def __init__(self, b):
        self.b, self.pos = b, 0

    def seek(self, off, whence=0):
        self.pos = off if whence == 0 else len(self.b) + off
        return self.pos

    def tell(self):
        return self.pos

    def read(self, n):
        out = self.b[self.pos:self.pos + n]
        self.pos += len(out)
        return out


class KeyFile:
    """A key file open for reading by offset.  `src`: a path, bytes, or a binary file object (seek, tell, read).
    The constructor reads and checks the header only; sections are read when asked for."""

    def __init__(self, src):
        self._own = None
        if isinstance(src, (bytes, bytearray, memoryview)):
            src = _Bytes(bytes(src))
        elif not hasattr(src, "read"):
            src = self._own = open(src, "rb")
        self.f = src
        self.size = self.f.seek(0, 2)
        head = self._read_at(0, min(HEADER_BYTES, self.size))
        if len(head) < 8:
            raise ValueError("header: truncated file (%d bytes)" % len(head))
        if head[:7] != MAGIC[:7]:
            raise ValueError("header: not a proving-key file (wrong magic)")
        if head[7] != MAGIC[7]:
            raise ValueError("header: key file version %d, this library reads version 1" % head[7])
        if len(head) < HEADER_BYTES:
            raise ValueError("header: truncated file (%d bytes, the header alone is %d)" % (len(head), HEADER_BYTES))
        ni, na, nc, m = struct.unpack_from("<IIII", head, 8)
        if m != _domain(nc, ni):
            raise ValueError("header: domain size %d, the counts say %d" % (m, _domain(nc, ni)))
        table = {}
        for i, name in enumerate(NAMES):
            sid, off, length = _ENTRY.unpack_from(head, 56 + 20 * i)
            if sid != i + 1:
                raise ValueError("header: section table entry %d has id %d, not %d (%s)" % (i, sid, i + 1, name))
            table[name] = (off, length)
        self.header = h = Header(ni, na, nc, m, head[24:56], table)
        spans = []
        for name, stride, count in SECTIONS:
            off, length = table[name]
            if off < HEADER_BYTES or off + length > self.size:
                raise ValueError("section %s: bytes [%d, %d) are out of bounds (header %d, file %d%s)"
                                 % (name, off, off + length, HEADER_BYTES, self.size,
                                    ": truncated file" if off + length > self.size else ""))
            if stride and length != stride * count(h):
                raise ValueError("section %s: %d bytes, the counts say %d x %d" % (name, length, count(h), stride))
            spans.append((off, off + length, name))
        spans.sort()
        for (_, end, a), (start, _, b) in zip(spans, spans[1:]):
            if start < end:
                raise ValueError("section %s overlaps section %s" % (b, a))

    def close(self):
        if self._own is not None:
            self._own.close()

    def _read_at(self, off, n):
        self.f.seek(off)
        out = self.f.read(n)
        if len(out) != n:
            raise ValueError("truncated file: %d bytes at offset %d, %d read" % (n, off, len(out)))
        return out

    def rows(self, name):
        return self.header.table[name][1] // STRIDE[name]

    def read(self, name, lo=None, hi=None) -> bytes:
        """A whole section, or rows [lo, hi) of a point array."""
        off, length = self.header.table[name]
        if lo is None:
            return self._read_at(off, length)
        s = STRIDE[name]
        if not 0 <= lo <= hi <= length // s:
            raise ValueError("section %s: rows [%d, %d) outside its %d" % (name, lo, hi, length // s))
        return self._read_at(off + lo * s, (hi - lo) * s)

    def read_joined(self, names, lo, hi):
        """Rows [lo, hi) of the concatenation of the point arrays `names` (one stride), read by offset:
        (bytes, [(name, first row of that array, count)] in the order of the bytes)."""
        out, parts, base = [], [], 0
        for name in names:
            n = self.rows(name)
            a, b = max(lo - base, 0), min(hi - base, n)
            if a < b:
                out.append(self.read(name, a, b))
                parts.append((name, a, b - a))
            base += n
        return b"".join(out), parts

    def verify_digest(self):
        """the SHA-256 of the header against every byte after the header"""
        if digest_from(self._read_at, HEADER_BYTES, self.size) != self.header.digest:
            raise ValueError("digest mismatch: the bytes after the header are not the ones the key was saved with")

    def r1cs(self):
        """((ptr, index, value) for A, B, C), strictly parsed"""
        h = self.header
        return tuple(parse_r1cs_section(name, self.read(name), h.num_constraints, h.nv)
                     for name in ("r1cs_a", "r1cs_b", "r1cs_c"))


def digest_from(read_at, off, size) -> bytes:
    """SHA-256 of the bytes [off, size) behind read_at(offset, count), 16 MiB at a time (the key file's digest, and
    the string file's of srs.py)"""
    sha = hashlib.sha256()
    while off < size:
        n = min(1 << 24, size - off)
        sha.update(read_at(off, n))
        off += n
    return sha.digest()


def locate(parts, j):
    """(name, index in that array) of row j of the bytes read_joined returned with `parts`"""
    for name, first, count in parts:
        if j < count:
            return name, first + j
        j -= count
    raise IndexError(j)
