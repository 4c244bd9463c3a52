"""A reader for the safetensors container, so checkpoints load without the `safetensors` package.

Layout: an 8-byte little-endian header length N, N bytes of JSON mapping each tensor name to
``{"dtype", "shape", "data_offsets": [begin, end]}`` (offsets relative to the end of the header; the optional
``"__metadata__"`` entry holds strings), then the raw little-endian tensor bytes.
"""
import json
import struct
from typing import Dict

import numpy as np
import torch

_NUMPY = {'F64': np.float64, 'F32': np.float32, 'F16': np.float16, 'I64': np.int64, 'I32': np.int32,
          'I16': np.int16, 'I8': np.int8, 'U8': np.uint8, 'BOOL': np.bool_}
_MAX_HEADER = 100 << 20


def load_safetensors(path: str) -> Dict[str, torch.Tensor]:
    """name -> CPU tensor (its stored dtype; BF16 as torch.bfloat16), in file-header order."""
    with open(path, 'rb') as f:
        head = f.read(8)
        if len(head) != 8:
            raise ValueError(f'{path}: not a safetensors file (shorter than its length field)')
        (n, ) = struct.unpack('<Q', head)
        if n <= 0 or n > _MAX_HEADER:
            raise ValueError(f'{path}: implausible safetensors header length {n}')
        raw = f.read(n)
        if len(raw) != n:
            raise ValueError(f'{path}: truncated safetensors header')
        header = json.loads(raw.decode('utf-8'))
        data = f.read()
    out = {}
    for name, info in header.items():
        if name == '__metadata__':
            continue
        dtype, shape = info['dtype'], tuple(int(s) for s in info['shape'])
        begin, end = (int(o) for o in info['data_offsets'])
        if not 0 <= begin <= end <= len(data):
            raise ValueError(f'{path}: tensor {name!r} lies outside the file')
        count = int(np.prod(shape)) if shape else 1
        if dtype == 'BF16':
            if end - begin != 2 * count:
                raise ValueError(f'{path}: tensor {name!r} has {end - begin} bytes, its shape needs {2 * count}')
            bits = np.frombuffer(data, dtype='<i2', count=count, offset=begin).copy()
            t = torch.from_numpy(bits).view(torch.bfloat16)
        elif dtype in _NUMPY:
            dt = np.dtype(_NUMPY[dtype]).newbyteorder('<')
            if end - begin != dt.itemsize * count:
                raise ValueError(f'{path}: tensor {name!r} has {end - begin} bytes, its shape needs '
                                 f'{dt.itemsize * count}')
            t = torch.from_numpy(np.frombuffer(data, dtype=dt, count=count, offset=begin).astype(_NUMPY[dtype]))
        else:
            raise ValueError(f'{path}: tensor {name!r} has unsupported dtype {dtype}')
        out[name] = t.reshape(shape)
    return out
