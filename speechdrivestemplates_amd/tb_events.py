"""TensorBoard event files without the ``tensorboard`` or ``tensorflow`` packages: the reference logs every learning
rate, loss, metric, figure and sample video to a SummaryWriter (core/pipelines/trainer.py:242-303, core/utils/video_processing.py:72-98);
``EventWriter`` writes the same records, so ``tensorboard --logdir <output dir>`` finds the run.

File: ``<log_dir>/events.out.tfevents.<10-digit unix time>.<hostname>``, a sequence of TFRecords
    uint64 LE length | uint32 LE masked_crc32c(length bytes) | data | uint32 LE masked_crc32c(data)
whose data are hand-encoded protobuf messages:
    Event          1 wall_time double, 2 step int64, 3 file_version string, 5 summary
    Summary        repeated 1 value
    Summary.Value  1 tag string, 2 simple_value float, 4 image, 5 histo
    Summary.Image  1 height, 2 width, 3 colorspace, 4 encoded_image_string
    HistogramProto 1 min, 2 max, 3 num, 4 sum, 5 sum_squares (doubles), 6 bucket_limit, 7 bucket (packed repeated doubles)
The first record is Event{wall_time, file_version: "brain.Event:2"}.  A GIF inside an image summary is what ``add_video`` produces.

    python -m speechdrivestemplates_amd.tb_events FILE [--extract DIR]
        one line per record: step, tag, then the value, ``image HxW <n> bytes`` or ``histogram num=... min=... max=... mean=... std=...
        buckets=...``; --extract writes the embedded PNG / GIF files, and every histogram as an .npz, to DIR
"""
import os
import socket
import struct
import time


def _crc_table():
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        table.append(c)
    return tuple(table)


_TABLE = _crc_table()


def crc32c(data):
    """CRC-32C (Castagnoli, reflected polynomial 0x82F63B78)"""
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = _TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def masked_crc32c(data):
    c = crc32c(data)
    return ((c >> 15 | c << 17) + 0xA282EAD8) & 0xFFFFFFFF


# -- protobuf encoding ----------------------------------------------------------------------------------------------------------------
def _varint(v):
    v &= (1 << 64) - 1  # negative int64: two's complement, 10 bytes
    out = bytearray()
    while v > 0x7F:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _key(field, wire):
    return _varint(field << 3 | wire)


def _f_varint(field, v):
    return _key(field, 0) + _varint(int(v))


def _f_bytes(field, data):
    data = data.encode("utf-8") if isinstance(data, str) else bytes(data)
    return _key(field, 2) + _varint(len(data)) + data


def _event(wall_time, step=None, file_version=None, summary=None):
    out = _key(1, 1) + struct.pack("<d", wall_time)
    if step is not None:
        out += _f_varint(2, step)
    if file_version is not None:
        out += _f_bytes(3, file_version)
    if summary is not None:
        out += _f_bytes(5, summary)
    return out


def scalar_summary(tag, value):
    return _f_bytes(1, _f_bytes(1, tag) + _key(2, 5) + struct.pack("<f", float(value)))


def image_summary(tag, encoded, height, width, colorspace=3):
    image = _f_varint(1, height) + _f_varint(2, width) + _f_varint(3, colorspace) + _f_bytes(4, encoded)
    return _f_bytes(1, _f_bytes(1, tag) + _f_bytes(4, image))


def histogram_summary(tag, min, max, num, sum, sum_squares, bucket_limit, bucket):
    """``bucket_limit``: the right edge of every bucket, ``bucket``: its count (tensor_hist.to_proto_fields makes both)"""
    bucket_limit, bucket = [float(x) for x in bucket_limit], [float(x) for x in bucket]
    if len(bucket_limit) != len(bucket):
        raise ValueError("a histogram has one limit per bucket, got %d limits and %d buckets" % (len(bucket_limit), len(bucket)))
    histo = b"".join(_key(i + 1, 1) + struct.pack("<d", float(v)) for i, v in enumerate((min, max, num, sum, sum_squares)))
    histo += _f_bytes(6, struct.pack("<%dd" % len(bucket_limit), *bucket_limit)) + _f_bytes(7, struct.pack("<%dd" % len(bucket), *bucket))
    return _f_bytes(1, _f_bytes(1, tag) + _f_bytes(5, histo))


def record(data):
    head = struct.pack("<Q", len(data))
    return head + struct.pack("<I", masked_crc32c(head)) + data + struct.pack("<I", masked_crc32c(data))


class EventWriter(object):
    """Appends records to one event file in ``log_dir``.  Thread-safe enough for its use here: every record is written with one call
    under a lock (the asynchronous video writer adds its GIFs from a worker thread)."""

    def __init__(self, log_dir):
        import threading
        os.makedirs(log_dir, exist_ok=True)
        now = time.time()
        self.path = os.path.join(log_dir, "events.out.tfevents.%010d.%s" % (int(now), socket.gethostname()))
        self._lock = threading.Lock()
        self._file = open(self.path, "ab")
        self._write(_event(now, file_version="brain.Event:2"))
        self.flush()

    def _write(self, event):
        with self._lock:
            if self._file is None:
                raise ValueError("the event file %s is closed" % self.path)
            self._file.write(record(event))

    def add_scalar(self, tag, value, step):
        self._write(_event(time.time(), step=int(step), summary=scalar_summary(tag, value)))

    def add_image_bytes(self, tag, encoded, height, width, step, colorspace=3):
        """an already encoded PNG or GIF file as an image summary"""
        self._write(_event(time.time(), step=int(step), summary=image_summary(tag, encoded, height, width, colorspace)))

    def add_histogram_raw(self, tag, min, max, num, sum, sum_squares, bucket_limit, bucket, step):
        """an already binned histogram (SummaryWriter.add_histogram_raw)"""
        self._write(_event(time.time(), step=int(step),
                           summary=histogram_summary(tag, min, max, num, sum, sum_squares, bucket_limit, bucket)))

    def flush(self):
        with self._lock:
            if self._file is not None:
                self._file.flush()

    def close(self):
        with self._lock:
            if self._file is not None:
                self._file.close()
                self._file = None


# -- reading (the inspection tool) ----------------------------------------------------------------------------------------------------
class CorruptFile(ValueError):
    pass


def _read_varint(buf, pos):
    v = shift = 0
    while True:
        if pos >= len(buf):
            raise CorruptFile("varint runs past the end of its message")
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        if not b & 0x80:
            return v, pos
        shift += 7
        if shift > 63:
            raise CorruptFile("varint longer than 10 bytes")


def _fields(buf):
    """protobuf message -> [(field, wire type, value)]: ints for varints, bytes for the rest"""
    pos, out = 0, []
    while pos < len(buf):
        k, pos = _read_varint(buf, pos)
        field, wire = k >> 3, k & 7
        if wire == 0:
            v, pos = _read_varint(buf, pos)
        elif wire in (1, 5):
            n = 8 if wire == 1 else 4
            v, pos = buf[pos:pos + n], pos + n
        elif wire == 2:
            n, pos = _read_varint(buf, pos)
            v, pos = buf[pos:pos + n], pos + n
        else:
            raise CorruptFile("unsupported wire type %d" % wire)
        if pos > len(buf):
            raise CorruptFile("field %d runs past the end of its message" % field)
        out.append((field, wire, v))
    return out


def read_records(path):
    """the data of every record; raises CorruptFile on a truncated record or a CRC mismatch"""
    with open(path, "rb") as f:
        buf = f.read()
    pos, out = 0, []
    while pos < len(buf):
        if pos + 12 > len(buf):
            raise CorruptFile("truncated record header at byte %d" % pos)
        n, = struct.unpack_from("<Q", buf, pos)
        if struct.unpack_from("<I", buf, pos + 8)[0] != masked_crc32c(buf[pos:pos + 8]):
            raise CorruptFile("length CRC mismatch at byte %d" % pos)
        if pos + 12 + n + 4 > len(buf):
            raise CorruptFile("truncated record at byte %d: %d bytes announced" % (pos, n))
        data = buf[pos + 12:pos + 12 + n]
        if struct.unpack_from("<I", buf, pos + 12 + n)[0] != masked_crc32c(data):
            raise CorruptFile("data CRC mismatch at byte %d" % pos)
        out.append(data)
        pos += 16 + n
    return out


def _doubles(wire, x):
    """a repeated double field: packed (wire type 2) or one element (wire type 1)"""
    if wire == 2 and len(x) % 8:
        raise CorruptFile("packed doubles of %d bytes" % len(x))
    return list(struct.unpack("<%dd" % (len(x) // 8), x)) if wire in (1, 2) else []


def _read_histo(buf):
    histo = {"min": 0.0, "max": 0.0, "num": 0.0, "sum": 0.0, "sum_squares": 0.0, "bucket_limit": [], "bucket": []}
    for f, w, x in _fields(buf):
        if w == 1 and 1 <= f <= 5:
            histo[("min", "max", "num", "sum", "sum_squares")[f - 1]], = struct.unpack("<d", x)
        elif f in (6, 7):
            histo["bucket_limit" if f == 6 else "bucket"] += _doubles(w, x)
    return histo


def read_events(path):
    """-> [{'wall_time', 'step', 'file_version' or None, 'values': [{'tag', 'simple_value'} | {'tag', 'image': {...}} |
    {'tag', 'histo': {'min', 'max', 'num', 'sum', 'sum_squares', 'bucket_limit', 'bucket'}}]}]"""
    events = []
    for data in read_records(path):
        ev = {"wall_time": None, "step": 0, "file_version": None, "values": []}
        for field, wire, v in _fields(data):
            if field == 1 and wire == 1:
                ev["wall_time"], = struct.unpack("<d", v)
            elif field == 2 and wire == 0:
                ev["step"] = v - (1 << 64) if v >> 63 else v
            elif field == 3 and wire == 2:
                ev["file_version"] = v.decode("utf-8")
            elif field == 5 and wire == 2:
                for f2, w2, value in _fields(v):
                    if f2 != 1 or w2 != 2:
                        continue
                    item = {"tag": None}
                    for f3, w3, x in _fields(value):
                        if f3 == 1 and w3 == 2:
                            item["tag"] = x.decode("utf-8")
                        elif f3 == 2 and w3 == 5:
                            item["simple_value"], = struct.unpack("<f", x)
                        elif f3 == 4 and w3 == 2:
                            img = {"height": 0, "width": 0, "colorspace": 0, "encoded": b""}
                            for f4, w4, y in _fields(x):
                                if w4 == 0 and f4 in (1, 2, 3):
                                    img[("height", "width", "colorspace")[f4 - 1]] = y
                                elif f4 == 4 and w4 == 2:
                                    img["encoded"] = bytes(y)
                            item["image"] = img
                        elif f3 == 5 and w3 == 2:
                            item["histo"] = _read_histo(x)
                    ev["values"].append(item)
        events.append(ev)
    return events


def describe(events):
    """the listing of the command-line tool, one line per record"""
    lines = []
    for ev in events:
        if ev["file_version"] is not None:
            lines.append("- file_version %s" % ev["file_version"])
        for item in ev["values"]:
            if "image" in item:
                img = item["image"]
                lines.append("%d %s image %dx%d %d bytes" % (ev["step"], item["tag"], img["height"], img["width"], len(img["encoded"])))
            elif "histo" in item:
                h = item["histo"]
                mean = h["sum"] / h["num"] if h["num"] else float("nan")
                std = max(h["sum_squares"] / h["num"] - mean * mean, 0.0) ** 0.5 if h["num"] else float("nan")
                lines.append("%d %s histogram num=%d min=%.9g max=%.9g mean=%.9g std=%.9g buckets=%d"
                             % (ev["step"], item["tag"], h["num"], h["min"], h["max"], mean, std, len(h["bucket"])))
            else:
                lines.append("%d %s %.9g" % (ev["step"], item["tag"], item.get("simple_value", float("nan"))))
    return lines


def _extension(encoded):
    return ".gif" if encoded[:6] in (b"GIF87a", b"GIF89a") else ".png" if encoded[:8] == b"\x89PNG\r\n\x1a\n" else ".bin"


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="list the records of a TensorBoard event file")
    ap.add_argument("file")
    ap.add_argument("--extract", metavar="DIR", help="write the embedded PNG and GIF files, and every histogram as an .npz, to DIR")
    a = ap.parse_args(argv)
    events = read_events(a.file)
    print("\n".join(describe(events)))
    if a.extract:
        os.makedirs(a.extract, exist_ok=True)
        n = 0
        for ev in events:
            for item in ev["values"]:
                if "image" in item:
                    enc = item["image"]["encoded"]
                    name = "%04d_step%d_%s%s" % (n, ev["step"], item["tag"].replace("/", "_"), _extension(enc))
                    with open(os.path.join(a.extract, name), "wb") as f:
                        f.write(enc)
                    n += 1
                elif "histo" in item:
                    import numpy as np
                    name = "%04d_step%d_%s.npz" % (n, ev["step"], item["tag"].replace("/", "_"))
                    np.savez(os.path.join(a.extract, name), **{k: np.asarray(v, dtype=np.float64) for k, v in item["histo"].items()})
                    n += 1
        print("extracted %d files to %s" % (n, a.extract))


if __name__ == "__main__":
    main()
