"""The checkpoint file of DQMC.save / DQMC.load (the place of save / load, FileIO.jl:38-156; the JLD container itself is
out of scope): one file with a JSON preamble, from which the object is constructed and configured again, and the engine's
state blob (dqmc_state_export, include/dqmc_hip.h "checkpoint and resume").

    8 bytes  b"DQMCCKPT"
    u32      container version (1)           little-endian
    u64      bytes of the preamble           "
    u64      bytes of the blob               "
    the preamble: UTF-8 JSON, one object
    the blob

Host code only: nothing here touches the device."""
import base64
import json
import os
import struct
import tempfile

import numpy as np

MAGIC = b"DQMCCKPT"
VERSION = 1
_HEAD = struct.Struct("<8sIQQ")


class CheckpointError(ValueError):
    pass


def join(preamble, blob):
    """-> the parts of the file as a list of bytes-like objects (the blob is not copied)"""
    if not isinstance(preamble, dict) or not preamble:
        raise CheckpointError("a checkpoint needs a preamble: a non-empty JSON object")
    blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    if blob.size == 0:
        raise CheckpointError("a checkpoint needs a state blob")
    text = json.dumps(preamble, sort_keys=True).encode("utf-8")
    return [_HEAD.pack(MAGIC, VERSION, len(text), blob.size), text, memoryview(blob)]


def split(data):
    """the bytes of a file -> (preamble dict, blob as a numpy.uint8 array); CheckpointError for anything that is not a
    whole checkpoint: another magic or version, a file cut short or with bytes behind its end, a preamble or a blob of
    no bytes (a preamble alone, a bare blob)"""
    data = memoryview(data).cast("B")
    if len(data) < _HEAD.size:
        raise CheckpointError("not a checkpoint: %d bytes do not hold the %d-byte head" % (len(data), _HEAD.size))
    magic, version, n_text, n_blob = _HEAD.unpack(data[:_HEAD.size])
    if magic != MAGIC:
        raise CheckpointError("not a checkpoint: the file does not start with %r" % (MAGIC,))
    if version != VERSION:
        raise CheckpointError("checkpoint container version %d, this package reads version %d" % (version, VERSION))
    if n_text == 0:
        raise CheckpointError("the checkpoint has no preamble")
    if n_blob == 0:
        raise CheckpointError("the checkpoint has no state blob")
    if len(data) != _HEAD.size + n_text + n_blob:
        raise CheckpointError("the checkpoint has %d bytes, its head describes %d" % (len(data), _HEAD.size + n_text + n_blob))
    try:
        preamble = json.loads(bytes(data[_HEAD.size:_HEAD.size + n_text]).decode("utf-8"))
    except ValueError as e:
        raise CheckpointError("the checkpoint's preamble is not JSON: %s" % e)
    if not isinstance(preamble, dict) or not preamble:
        raise CheckpointError("the checkpoint's preamble is not a non-empty JSON object")
    return preamble, np.frombuffer(data[_HEAD.size + n_text:], dtype=np.uint8).copy()


def write_atomic(path, parts):
    """writes the parts to a temporary file in the directory of `path`, then os.replace: a reader sees the old file or the
    new one, never a part of either.  If anything raises, the temporary is removed and `path` is as it was."""
    path = os.fspath(path)
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(path) or ".")
    try:
        with os.fdopen(fd, "wb") as f:
            for part in parts:
                f.write(part)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def write(path, preamble, blob):
    write_atomic(path, join(preamble, blob))


def read(path):
    with open(path, "rb") as f:
        return split(f.read())


def pack_table(a):
    """an integer table -> a JSON value that gives back the same int32 array (unpack_table)"""
    a = np.ascontiguousarray(a, dtype="<i4")
    return {"shape": list(a.shape), "int32": base64.b64encode(a.tobytes()).decode("ascii")}


def unpack_table(d):
    a = np.frombuffer(base64.b64decode(d["int32"]), dtype="<i4").astype(np.int32)
    return a.reshape(tuple(d["shape"]))
