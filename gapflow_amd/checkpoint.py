"""Checkpoint files: the device blob of libgapflow_hip (gpf_checkpoint_save) behind a small header of the host's own.

    b'GPFCKPTF' | uint32 format version | uint64 n | n bytes of JSON (UTF-8) | uint64 m | m bytes of blob

The JSON holds the sanitised input dictionaries as text (options, grid, numerics, properties, geometry) and the host-side mirror
of the run (history, residual_buffer, kinetic_energy_old, ...); everything the next step depends on is in the blob (DESIGN.md
3.3d).  Files are written to ``path + '.tmp'`` and moved into place with ``os.replace``: a run ended in the middle of a write
leaves the previous checkpoint intact.
"""
import ctypes as C
import json
import os
import struct

import numpy as np

from . import _lib

MAGIC = b'GPFCKPTF'
VERSION = 1
_HEAD = struct.Struct('<8sIQ')
_LEN = struct.Struct('<Q')
INPUT_KEYS = ('options', 'grid', 'numerics', 'properties', 'geometry')
NOT_SAVED = {
    'surrogate': "checkpoint: surrogate problems (database, hyper-parameters and the Mock runner's random stream) are not saved yet",
    'elastic slab': "checkpoint: elastic slabs (the distributed transform's under-relaxation state) are not saved yet",
    'random asperities on slabs': "checkpoint: slabs of a gap with randomly drawn asperity heights (num > 1) are not saved yet",
}


def _plain(o):
    """NumPy scalars and arrays, tuples and deques of the sanitised dictionaries as JSON values (floats survive: repr round-trips)."""
    if isinstance(o, dict):
        return {str(k): _plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)) or type(o).__name__ == 'deque':
        return [_plain(v) for v in o]
    if isinstance(o, np.ndarray):
        return _plain(o.tolist())
    if isinstance(o, np.generic):
        return o.item()
    return o


def input_dicts(options, grid, numerics, prop, geo):
    return _plain(dict(zip(INPUT_KEYS, (options, grid, numerics, prop, geo))))


def pack(meta, blob):
    text = json.dumps(_plain(meta)).encode('utf-8')
    blob = bytes(blob) if not isinstance(blob, (bytes, bytearray, memoryview)) else blob
    return b''.join([_HEAD.pack(MAGIC, VERSION, len(text)), text, _LEN.pack(len(blob)), blob])


def unpack(data):
    """-> (meta, blob) of the bytes of a checkpoint file; ValueError for anything that is not a whole file of this format."""
    if len(data) < _HEAD.size:
        raise ValueError("checkpoint: truncated file (shorter than its header)")
    magic, version, n = _HEAD.unpack_from(data, 0)
    if magic != MAGIC:
        raise ValueError("checkpoint: not a gapflow_amd checkpoint file (magic differs)")
    if version != VERSION:
        raise ValueError(f"checkpoint: file format version {version}, this build reads version {VERSION}")
    at = _HEAD.size
    if len(data) < at + n + _LEN.size:
        raise ValueError("checkpoint: truncated file (input dictionaries incomplete)")
    try:
        meta = json.loads(bytes(data[at:at + n]).decode('utf-8'))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise ValueError(f"checkpoint: damaged file header ({e})") from None
    at += n
    m, = _LEN.unpack_from(data, at)
    at += _LEN.size
    if len(data) != at + m:
        raise ValueError(f"checkpoint: truncated file ({len(data) - at} of {m} bytes of device state)")
    return meta, data[at:at + m]


def write_file(path, meta, blob):
    """Atomic: the bytes go to path + '.tmp', which then replaces path."""
    tmp = path + '.tmp'
    with open(tmp, 'wb') as f:
        f.write(pack(meta, blob))
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def read_file(path):
    with open(path, 'rb') as f:
        return unpack(f.read())


def device_blob(lib, handle):
    """gpf_checkpoint_save of a handle into a NumPy byte array."""
    n = C.c_size_t(0)
    _lib.check(lib.gpf_checkpoint_size(handle, C.byref(n)))
    buf = np.empty(n.value, dtype=np.uint8)
    written = C.c_size_t(0)
    _lib.check(lib.gpf_checkpoint_save(handle, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(written)))
    return buf[:written.value]


def load_device_blob(lib, handle, blob):
    """gpf_checkpoint_load; GapflowHipError (a RuntimeError) names what the library refused and the handle stays as it was."""
    buf = np.frombuffer(blob, dtype=np.uint8)
    buf = np.require(buf, requirements=['C', 'A'])
    _lib.check(lib.gpf_checkpoint_load(handle, buf.ctypes.data_as(C.c_void_p), buf.size))


def rank_path(path, rank):
    return f"{path}.rank{rank:03d}"
