"""Guard-band allocator for the extent tests (tests/test_gpu_extents.py, self-tested on the CPU in tests/test_cpu_arena.py).

GPU address sanitizers are not available to this project, so *where* a kernel touches memory is watched from the outside:
every operand of a call is carved from ONE ``uint8`` allocation (an :class:`Arena`) with a guard band on each side and, when
its row stride ``ld`` exceeds the row length, spare columns in every row.  Guards and spare columns hold a byte pattern;
after the call :meth:`Arena.check` compares every such byte with the pattern and every ``role="input"`` buffer with the
snapshot :meth:`Arena.arm` took before the call.  The pattern is a parameter, so the same case can run in two surroundings
(``0x00`` and ``0xFF`` = NaN as fp32 / fp16, -1 as int32, 255 as uint8): a result that depends on memory outside the
documented extent differs between the two runs.

What it cannot see: a READ outside an extent that does not influence any result (only a fault would show it), and stores
farther away than the guard (at least max(64 KiB, 256 rows x row pitch) per side: the largest tile here is 256 rows).

Plain helper module, device agnostic (CPU tensors work the same way), no pytest hooks.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

GUARD_MIN_BYTES = 64 << 10
GUARD_MIN_ROWS = 256
ALT_PATTERN = 0x7F            # used around an integer buffer whose contract names a filler equal to the arena's pattern
ROLES = ("input", "output", "inout", "workspace")


class GuardViolation(AssertionError):
    pass


def _prod(xs: Sequence[int]) -> int:
    n = 1
    for x in xs:
        n *= int(x)
    return n


def pattern_value(pattern: int, dtype: torch.dtype):
    """The element a buffer of ``dtype`` shows where every byte is ``pattern``."""
    n = torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), pattern, dtype=torch.uint8).view(dtype)[0].item()


@dataclass
class Buffer:
    name: str
    role: str
    dtype: torch.dtype
    shape: Tuple[int, ...]
    rows: int
    row_bytes: int            # payload bytes per row
    pitch: int                # bytes from one row to the next
    start: int                # arena offset of the first payload byte
    guard: int                # guard bytes on each side
    pattern: int
    view: torch.Tensor = field(repr=False, default=None)
    snapshot: Optional[torch.Tensor] = field(repr=False, default=None)
    row_off: Optional[torch.Tensor] = field(repr=False, default=None)   # byte offset of every payload row from start (ascending)

    @property
    def end(self) -> int:     # one past the last payload byte
        return self.start + int(self.row_off[-1]) + self.row_bytes if self.rows else self.start

    @property
    def nbytes(self) -> int:  # documented extent when the rows are dense (pitch == row_bytes)
        return self.end - self.start


class Arena:
    """``Arena(capacity_bytes, device, pattern)``: a bump allocator over one pattern-filled ``uint8`` tensor."""

    def __init__(self, capacity: int, device="cpu", pattern: int = 0x00):
        if not 0 <= pattern <= 255:
            raise ValueError("pattern is one byte")
        self.pattern = int(pattern)
        self.device = torch.device(device)
        self.capacity = int(capacity) + 4096
        self.mem = torch.full((self.capacity,), self.pattern, dtype=torch.uint8, device=self.device)
        self._base = (-self.mem.data_ptr()) % 4096          # arena offsets are relative to a 4 KiB aligned address
        self._top = self._base
        self.buffers: Dict[str, Buffer] = {}
        self.armed = False

    # ---------------------------------------------------------------------------------------------- allocation
    def take(self, name: str, shape, dtype: torch.dtype = torch.float32, *, ld: Optional[int] = None, align: int = 256,
             misalign: int = 0, role: str = "output", fillers: Sequence[int] = (), fill: Optional[int] = None,
             data: Optional[torch.Tensor] = None, batch_stride: Optional[int] = None, row_pitch: Optional[int] = None,
             guard_bytes: Optional[int] = None) -> torch.Tensor:
        """A view of ``shape`` / ``dtype`` whose rows (the last dimension) are ``ld`` elements apart (default: dense).

        ``batch_stride`` (3-d shapes [B, R, C] only): image b starts ``batch_stride`` ROWS after image b - 1 (the
        ``c_batch_stride`` outputs); the rows between two images are watched like spare columns.
        ``align`` / ``misalign``: the view's address is ``misalign`` modulo ``align`` — pass the weakest alignment the
        contract allows so that the unaligned code paths run.  ``fillers``: values the contract of an integer output
        names as filler (``-1`` index rows): when the arena's pattern shows as one of them in ``dtype`` the guards of this
        buffer use ``ALT_PATTERN`` instead, so that a stray filler store still differs from the guard.  ``fill``: byte the
        payload starts with (default: the guard pattern); ``data``: initial contents (copied into the view).
        ``row_pitch`` (1-d byte blobs such as a split weight buffer or a workspace): bytes of one logical row of what the
        blob holds, for sizing the guard (256 rows of it); a 1-d buffer without it gets the 64 KiB minimum.
        ``guard_bytes``: the guard on each side in bytes (rounded up to 256) INSTEAD of the default — wider where the case watches
        for far strays (tests/test_gpu_offsets.py: 2 GiB, so that an address wrapped at 2^31 or 2^32 still lands in memory the
        arena owns), or narrower where 256 rows of a very wide pitch would not fit a device.  Guards of that size are checked
        with :meth:`check_blocked`."""
        if role not in ROLES:
            raise ValueError(f"role must be one of {ROLES}")
        if name in self.buffers:
            raise ValueError(f"buffer {name!r} taken twice")
        if self.armed:
            raise RuntimeError("take() after arm(): carve every operand first")
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        esz = torch.empty((), dtype=dtype).element_size()
        cols = shape[-1] if shape else 1
        rows = _prod(shape[:-1])
        if rows * cols <= 0:
            raise ValueError(f"{name}: empty buffer")
        ld = cols if ld is None else int(ld)
        if ld < cols:
            raise ValueError(f"{name}: ld {ld} < row length {cols}")
        if misalign % esz or align % esz or not 0 <= misalign < align or 4096 % align:
            raise ValueError(f"{name}: align {align} / misalign {misalign} do not fit {esz}-byte elements")
        pattern = self.pattern
        if fillers:
            if dtype.is_floating_point:
                raise ValueError("fillers are for integer buffers")
            if pattern_value(pattern, dtype) in set(int(f) for f in fillers):
                pattern = ALT_PATTERN
            if pattern_value(pattern, dtype) in set(int(f) for f in fillers):
                raise ValueError(f"{name}: no pattern differs from the fillers {tuple(fillers)}")
        pitch, row_bytes = ld * esz, cols * esz
        strides = []
        s = ld
        for d in reversed(shape[:-1]):
            strides.append(s)
            s *= d
        strides = tuple(reversed(strides)) + (1,)
        if batch_stride is not None:
            if len(shape) != 3 or batch_stride < shape[1]:
                raise ValueError(f"{name}: batch_stride needs a [B, R, C] shape and at least R rows")
            strides = (int(batch_stride) * ld, ld, 1)
        # byte offset of every payload row
        row_idx = torch.zeros((), dtype=torch.int64)
        for d, st in zip(shape[:-1], strides[:-1]):
            row_idx = row_idx[..., None] + torch.arange(d, dtype=torch.int64) * st
        row_off = (row_idx.reshape(-1) * esz).to(self.device)
        guard = max(GUARD_MIN_BYTES, GUARD_MIN_ROWS * (pitch if len(shape) > 1 else int(row_pitch or 0)))
        if guard_bytes is not None:
            if guard_bytes < 0:
                raise ValueError(f"{name}: guard_bytes {guard_bytes} < 0")
            guard = int(guard_bytes)
        guard = (guard + 255) // 256 * 256
        start = self._top + guard
        start += (misalign - (start - self._base)) % align
        buf = Buffer(name, role, dtype, shape, rows, row_bytes, pitch, start, guard, pattern, row_off=row_off)
        top = buf.end + guard
        if top > self.capacity:
            raise MemoryError(f"arena of {self.capacity} bytes exhausted by {name!r} (needs {top}): raise the capacity")
        self._top = top
        if pattern != self.pattern:
            self.mem[start - guard:top] = pattern
        # typed view over the payload and what lies between its rows (guard bytes are never written through it)
        typed = self.mem[start:start + (buf.end - start + esz - 1) // esz * esz].view(dtype)
        view = typed.as_strided(shape, strides)
        buf.view = view
        if fill is not None:
            self._put(buf, torch.full((rows, row_bytes), fill, dtype=torch.uint8, device=self.device))
        if data is not None:
            view.copy_(data.to(self.device).reshape(shape))
        self.buffers[name] = buf
        return view

    def _index(self, buf: Buffer) -> torch.Tensor:
        """[rows, row_bytes] arena offsets of the payload bytes."""
        return buf.start + buf.row_off[:buf.rows, None] + torch.arange(buf.row_bytes, device=self.device)[None, :]

    @staticmethod
    def _dense(buf: Buffer) -> bool:
        """One contiguous run of bytes (large buffers then need no index tensors)."""
        return buf.rows == 1 or (buf.pitch == buf.row_bytes and int(buf.row_off[-1]) == (buf.rows - 1) * buf.pitch)

    def _get(self, buf: Buffer) -> torch.Tensor:
        if self._dense(buf):
            return self.mem[buf.start:buf.end].clone().view(buf.rows, buf.row_bytes)
        return self.mem[self._index(buf)]

    def _put(self, buf: Buffer, rows_u8: torch.Tensor) -> None:
        if self._dense(buf):
            self.mem[buf.start:buf.end] = rows_u8.reshape(-1)
        else:
            self.mem[self._index(buf)] = rows_u8

    def payload_bytes(self, name: str) -> torch.Tensor:
        """A copy of the payload bytes [rows, row_bytes] (for bit comparisons of outputs between two runs)."""
        return self._get(self.buffers[name])

    # ---------------------------------------------------------------------------------------------- arm / check
    def arm(self) -> None:
        """Snapshot every ``role="input"`` buffer: call after the operands are filled, right before the launch."""
        for buf in self.buffers.values():
            if buf.role == "input":
                buf.snapshot = self._get(buf)
        self.armed = True

    def shrink(self, name: str, *, rows: int = 0, cols: int = 0, tail_bytes: int = 0) -> None:
        """Declare the extent of ``name`` SMALLER than it was taken (sensitivity tests only): the dropped rows / columns /
        trailing bytes are re-filled with the pattern and watched like guard bytes.  The view keeps its shape."""
        buf = self.buffers[name]
        esz = torch.empty((), dtype=buf.dtype).element_size()
        if rows:
            buf.rows -= rows
            buf.row_off = buf.row_off[:buf.rows]
        if cols:
            buf.row_bytes -= cols * esz
        if tail_bytes:
            if buf.rows != 1 and buf.pitch != buf.row_bytes:
                raise ValueError("tail_bytes is for dense buffers")
            buf.row_bytes = buf.rows * buf.row_bytes - tail_bytes
            buf.rows, buf.pitch, buf.row_off = 1, buf.row_bytes, buf.row_off[:1]
        keep = self._get(buf)
        self.mem[buf.start:buf.start + (buf.end - buf.start) + (rows * buf.pitch + cols * esz + tail_bytes)] = buf.pattern
        self._put(buf, keep)
        if buf.snapshot is not None:
            buf.snapshot = keep

    def violations(self) -> List[dict]:
        """Every guard / spare-column / input violation as a dict (empty list = clean).  Synchronise the device first."""
        out = []
        for buf in self.buffers.values():
            lo, span = buf.start - buf.guard, buf.end - buf.start
            region = self.mem[lo:buf.end + buf.guard]
            if self._dense(buf):
                bad = torch.cat([(region[:buf.guard] != buf.pattern).nonzero().flatten(),
                                 (region[buf.guard + span:] != buf.pattern).nonzero().flatten() + buf.guard + span])
            else:
                watched = torch.ones(region.numel(), dtype=torch.bool, device=self.device)
                watched[self._index(buf).reshape(-1) - lo] = False
                bad = ((region != buf.pattern) & watched).nonzero().flatten()
            if bad.numel():
                low = bad[bad < buf.guard]
                high = bad[bad >= buf.guard + span] - (buf.guard + span)
                mid = bad[(bad >= buf.guard) & (bad < buf.guard + span)] - buf.guard
                if low.numel():       # distance d >= 1 from the edge: the byte at start - d
                    d = buf.guard - low
                    out.append(dict(buffer=buf.name, side="low guard", first=int(d.min()), last=int(d.max()), count=int(low.numel())))
                if high.numel():      # distance d >= 1: the byte at end - 1 + d
                    out.append(dict(buffer=buf.name, side="high guard", first=int(high.min()) + 1, last=int(high.max()) + 1,
                                    count=int(high.numel())))
                if mid.numel():       # (payload row before it, bytes past that row's last payload byte, 1-based)
                    row = torch.searchsorted(buf.row_off, mid, right=True) - 1
                    col = mid - buf.row_off[row] - buf.row_bytes + 1
                    out.append(dict(buffer=buf.name, side="spare columns", first=(int(row[0]), int(col[0])),
                                    last=(int(row[-1]), int(col[-1])), count=int(mid.numel())))
            if buf.snapshot is not None:
                bad = (self._get(buf) != buf.snapshot).nonzero()
                if bad.shape[0]:      # (row, byte offset inside the row)
                    first, last = bad[0], bad[-1]
                    out.append(dict(buffer=buf.name, side="input changed", first=(int(first[0]), int(first[1])),
                                    last=(int(last[0]), int(last[1])), count=int(bad.shape[0])))
        return out

    # ---------------------------------------------------------------------------------------------- multi-GiB arenas
    def _scan(self, lo: int, hi: int, pattern: int, block: int) -> Optional[int]:
        """Arena offset of the first byte of [lo, hi) that differs from ``pattern`` (None: clean), ``block`` bytes at a time."""
        for a in range(lo, hi, block):
            chunk = self.mem[a:min(a + block, hi)]
            head = (-a) % 8                                   # whole 8-byte words in the middle: an eighth of the elements
            if chunk.numel() >= 64 and (chunk.data_ptr() + head) % 8 == 0:
                body = chunk[head:head + (chunk.numel() - head) // 8 * 8].view(torch.int64)
                word = int.from_bytes(bytes([pattern]) * 8, "little", signed=True)
                if bool((body == word).all()) and bool((chunk[:head] == pattern).all()) and \
                        bool((chunk[head + body.numel() * 8:] == pattern).all()):
                    continue
            elif bool((chunk == pattern).all()):
                continue
            return a + int((chunk != pattern).nonzero()[0])
        return None

    def violations_blocked(self, block_bytes: int = 256 << 20) -> List[dict]:
        """What :meth:`violations` reports — guards, spare columns, rows between images, changed inputs — found without index or
        mask tensors of the arena's size: guards and gaps are walked ``block_bytes`` at a time, spare columns as strided views over
        blocks of rows.  For arenas of several GiB, where the masks of :meth:`violations` would not fit beside the arena.  One
        record per buffer and side, with the first offending byte only (``count`` is 1: the walk stops there)."""
        out = []
        for buf in self.buffers.values():
            def rec(side, first):
                out.append(dict(buffer=buf.name, side=side, first=first, last=first, count=1))
            bad = self._scan(buf.start - buf.guard, buf.start, buf.pattern, block_bytes)
            if bad is not None:                               # the LAST bad byte is the nearest; report the first found, as a distance
                rec("low guard", buf.start - bad)
            bad = self._scan(buf.end, buf.end + buf.guard, buf.pattern, block_bytes)
            if bad is not None:
                rec("high guard", bad - buf.end + 1)
            if buf.rows > 1:
                off = buf.row_off[:buf.rows].cpu()
                step = off[1:] - off[:-1]
                cut = (step != buf.pitch).nonzero().flatten().tolist()            # rows after which the pitch is irregular
                spare = buf.pitch - buf.row_bytes
                r0 = 0
                for r1 in cut + [buf.rows - 1]:                                   # rows r0 .. r1 are one pitch apart
                    n = r1 - r0                                                   # spare runs behind rows r0 .. r1 - 1
                    per = max(1, block_bytes // max(spare, 1))
                    for a in range(0, n if spare else 0, per):
                        k = min(per, n - a)
                        base = buf.start + int(off[r0 + a]) + buf.row_bytes
                        v = self.mem.as_strided((k, spare), (buf.pitch, 1), base + self.mem.storage_offset())
                        if not bool((v == buf.pattern).all()):
                            rc = (v != buf.pattern).nonzero()[0]
                            rec("spare columns", (r0 + a + int(rc[0]), int(rc[1]) + 1))
                            break
                    if r1 < buf.rows - 1:                                         # the gap up to the next run (rows between images)
                        lo = buf.start + int(off[r1]) + buf.row_bytes
                        bad = self._scan(lo, buf.start + int(off[r1 + 1]), buf.pattern, block_bytes)
                        if bad is not None:
                            rec("spare columns", (r1, bad - lo + 1))
                    r0 = r1 + 1
            if buf.snapshot is not None:
                diff = (self._get(buf) != buf.snapshot).nonzero()
                if diff.shape[0]:
                    first = diff[0]
                    rec("input changed", (int(first[0]), int(first[1])))
        return out

    def check_blocked(self, block_bytes: int = 256 << 20) -> None:
        if not self.armed:
            raise RuntimeError("check_blocked() without arm()")
        v = self.violations_blocked(block_bytes)
        if v:
            lines = [f"{r['buffer']}: {r['side']}: first offending byte at {r['first']}" for r in v]
            raise GuardViolation("memory touched outside the documented extents (guards: 1-based distance from the payload "
                                 "edge; spare columns: (row, bytes past the row's end); inputs: (row, byte)):\n  " + "\n  ".join(lines))

    def check(self) -> None:
        if not self.armed:
            raise RuntimeError("check() without arm()")
        v = self.violations()
        if v:
            lines = [f"{r['buffer']}: {r['side']}: {r['count']} byte(s), first at {r['first']}, last at {r['last']}" for r in v]
            raise GuardViolation("memory touched outside the documented extents (guards: 1-based distance from the payload "
                                 "edge; spare columns: (row, bytes past the row's end); inputs: (row, byte)):\n  " + "\n  ".join(lines))
