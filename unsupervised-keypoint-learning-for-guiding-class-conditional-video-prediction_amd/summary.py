"""TensorBoard event files without TensorFlow: the ``tf.summary.FileWriter`` of the reference's two training modes
(models/base_model.py:62-75, detector_translator_model.py:84-141 / 205-244, motion_generator_model.py:80-145 / 217-276).

Formats restated from their public definitions (TF 1.12 semantics, DESIGN.md section 2 [TF-sem]):

* an event file ``<logdir>/events.out.tfevents.%010d.<hostname>`` is a sequence of TFRecord frames: u64 length, masked CRC-32C of the
  length bytes, the data, masked CRC-32C of the data (lib/io/record_writer.cc); the first record is ``Event{wall_time, file_version=
  "brain.Event:2"}``;
* ``Event`` (util/event.proto): wall_time = 1 (double), step = 2 (int64), file_version = 3 (string), summary = 5 (Summary); proto3, so a
  zero step is not written;
* ``Summary`` (framework/summary.proto): repeated value = 1; ``Value``: tag = 1, simple_value = 2 (float), image = 4;
  ``Image``: height = 1, width = 2, colorspace = 3 (= channels), encoded_image_string = 4 (PNG).

The float -> uint8 conversion of an image summary runs on the GPU (``ops.summary_image_u8``); this module only frames and encodes.
``read_events`` reads the files back (every checksum verified), so the scalars can be dumped without TensorBoard.
"""
import os
import socket
import struct
import time
import zlib

import numpy as np

from .tf_bundle import _pb_fields, _varint, crc32c, mask_crc, unmask_crc

FILE_VERSION = 'brain.Event:2'


# ------------------------------------------------------------------------------------------------ protobuf fragments
def _key(field, wire_type):
    return _varint((field << 3) | wire_type)


def _bytes_field(field, data):
    return _key(field, 2) + _varint(len(data)) + data


def scalar_value(tag, value):
    """``Summary.Value{tag, simple_value}`` (tf.summary.scalar; the value is stored as fp32)."""
    return _bytes_field(1, tag.encode()) + _key(2, 5) + struct.pack('<f', float(value))


def encode_png(img):
    """uint8 [H,W,C] (C = 1 gray, 3 RGB, 4 RGBA) -> PNG bytes: 8-bit, filter 0 on every row, one zlib IDAT chunk."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, c = img.shape
    if c not in (1, 3, 4) or h < 1 or w < 1:
        raise ValueError('encode_png: uint8 [H,W,C] with C in (1, 3, 4) (got %s)' % (img.shape,))
    color_type = {1: 0, 3: 2, 4: 6}[c]
    rows = np.zeros((h, 1 + w * c), dtype=np.uint8)
    rows[:, 1:] = img.reshape(h, w * c)

    def chunk(kind, data):
        return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, color_type, 0, 0, 0))
            + chunk(b'IDAT', zlib.compress(rows.tobytes())) + chunk(b'IEND', b''))


def image_values(name, images, max_outputs=2):
    """``Summary.Value`` entries of tf.summary.image(name, ..., max_outputs) from the already converted uint8 [N,H,W,C] images (the first
    ``max_outputs`` are used): tag ``name/image/i`` when max_outputs > 1, ``name/image`` otherwise (SummaryImageOp)."""
    images = np.asarray(images)
    if images.ndim != 4 or images.dtype != np.uint8:
        raise ValueError('image_values: uint8 [N,H,W,C] expected (got %s %s)' % (images.shape, images.dtype))
    out = []
    for i in range(min(images.shape[0], max_outputs)):
        tag = '%s/image/%d' % (name, i) if max_outputs > 1 else '%s/image' % name
        _, h, w, c = images.shape
        img = (_key(1, 0) + _varint(h) + _key(2, 0) + _varint(w) + _key(3, 0) + _varint(c)
               + _bytes_field(4, encode_png(images[i])))
        out.append(_bytes_field(1, tag.encode()) + _bytes_field(4, img))
    return out


def encode_event(wall_time, step=0, values=None, file_version=None):
    out = _key(1, 1) + struct.pack('<d', float(wall_time))
    if step:
        out += _key(2, 0) + _varint(int(step))
    if file_version is not None:
        out += _bytes_field(3, file_version.encode())
    if values is not None:
        out += _bytes_field(5, b''.join(_bytes_field(1, v) for v in values))
    return out


def frame_record(data):
    """One TFRecord frame."""
    length = struct.pack('<Q', len(data))
    return length + struct.pack('<I', mask_crc(crc32c(length))) + data + struct.pack('<I', mask_crc(crc32c(data)))


# ------------------------------------------------------------------------------------------------ writer
class EventFileWriter(object):
    """``tf.summary.FileWriter(logdir)`` without the graph: ``add_summary(values, step)`` appends one Event holding the given
    ``Summary.Value`` entries (one merged summary = one call).  Every event is flushed to the file as it is written."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        self.logdir = logdir
        self.path = os.path.join(logdir, 'events.out.tfevents.%010d.%s' % (int(time.time()), socket.gethostname()))
        self._f = open(self.path, 'ab')
        self._write(encode_event(time.time(), file_version=FILE_VERSION))

    def _write(self, data):
        self._f.write(frame_record(data))
        self._f.flush()

    def add_summary(self, values, step):
        if self._f is None:
            raise ValueError('EventFileWriter: add_summary after close()')
        self._write(encode_event(time.time(), step=step, values=list(values)))

    def flush(self):
        if self._f is not None:
            self._f.flush()

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None


# ------------------------------------------------------------------------------------------------ reader
def read_records(path):
    """The data of every TFRecord frame of ``path``; raises ValueError on a checksum mismatch or a truncated frame."""
    with open(path, 'rb') as f:
        buf = f.read()
    pos, out = 0, []
    while pos < len(buf):
        if pos + 12 > len(buf):
            raise ValueError('%s: truncated record header at byte %d' % (path, pos))
        length = buf[pos:pos + 8]
        n = struct.unpack('<Q', length)[0]
        if unmask_crc(struct.unpack_from('<I', buf, pos + 8)[0]) != crc32c(length):
            raise ValueError('%s: length checksum mismatch at byte %d' % (path, pos))
        if pos + 12 + n + 4 > len(buf):
            raise ValueError('%s: truncated record at byte %d' % (path, pos))
        data = buf[pos + 12:pos + 12 + n]
        if unmask_crc(struct.unpack_from('<I', buf, pos + 12 + n)[0]) != crc32c(data):
            raise ValueError('%s: data checksum mismatch at byte %d' % (path, pos))
        out.append(data)
        pos += 12 + n + 4
    return out


def _decode_value(buf):
    v = {}
    for field, _, val in _pb_fields(buf):
        if field == 1:
            v['tag'] = val.decode()
        elif field == 2:
            v['simple_value'] = struct.unpack('<f', struct.pack('<I', val))[0]
        elif field == 4:
            img = {'height': 0, 'width': 0, 'colorspace': 0, 'encoded_image_string': b''}
            for f2, _, x in _pb_fields(val):
                img[{1: 'height', 2: 'width', 3: 'colorspace', 4: 'encoded_image_string'}.get(f2, f2)] = x
            v['image'] = img
    return v


def read_events(path):
    """-> list of dicts {'wall_time', 'step', 'file_version' (or None), 'values': [{'tag', 'simple_value' | 'image'}]}, in file order."""
    events = []
    for data in read_records(path):
        e = {'wall_time': 0.0, 'step': 0, 'file_version': None, 'values': []}
        for field, _, val in _pb_fields(data):
            if field == 1:
                e['wall_time'] = struct.unpack('<d', struct.pack('<Q', val))[0]
            elif field == 2:
                e['step'] = val - (1 << 64) if val >> 63 else val
            elif field == 3:
                e['file_version'] = val.decode()
            elif field == 5:
                e['values'] = [_decode_value(v) for f2, _, v in _pb_fields(val) if f2 == 1]
        events.append(e)
    return events


def scalars(path):
    """{tag: [(step, value), ...]} of every scalar in an event file, or -- given a directory -- in all its event files, oldest first
    (a run resumed with train.py --resume opens new files beside those of the runs before it)."""
    out = {}
    for p in (event_files(path) if os.path.isdir(path) else [path]):
        for e in read_events(p):
            for v in e['values']:
                if 'simple_value' in v:
                    out.setdefault(v['tag'], []).append((e['step'], v['simple_value']))
    return out


def event_files(logdir):
    """The event files of ``logdir``, oldest first."""
    return sorted(os.path.join(logdir, f) for f in os.listdir(logdir) if f.startswith('events.out.tfevents.'))


def image_summary(items, max_outputs=2):
    """The ``Summary.Value`` entries of one merged image summary: ``items`` = [(name, fp32 [N,H,W,C] device tensor, premap), ...] in merge
    order.  Every conversion is launched (ops.summary_image_u8, first ``max_outputs`` images) before the one host copy of each result."""
    from . import ops
    u8 = [(name, ops.summary_image_u8(x, premap, max_outputs=max_outputs)) for name, x, premap in items]
    values = []
    for name, t in u8:
        values += image_values(name, t.cpu().numpy(), max_outputs=max_outputs)
    return values
