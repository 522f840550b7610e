"""Input feed of the inference scripts -- mirror of `lib_yolo/dataset_utils.py` `TestingDataset`
(:188-219) and `decode_img` (:6-11), without TensorFlow:

  TFRecord framing   u64 length | u32 masked-crc32c(length) | payload | u32 masked-crc32c(payload)
  payload            a `tf.train.Example` protobuf; features read (schema written by
                     `create_tf_records_citypersons.py:132-147`): `image/encoded` (PNG bytes),
                     `image/filename`, `image/height`, `image/width`
  image              PNG -> uint8 HWC -> float32 * (1/255)   (tf.image.convert_image_dtype)

The reference's pipeline (:190-199) is  list_files -> interleave(TFRecordDataset, cycle_length=2, block_length=1) ->
map(parse_example, num_parallel_calls=config['cpu_thread_cnt']) -> batch -> prefetch(1).  Here:

  * records are taken in sorted file order, interleaved two files at a time (the reference's `list_files` order is shuffled
    and therefore not reproducible);
  * the map stage runs on `cpu_thread_cnt` native threads (csrc/host_io.cpp through the C-ABI: byolo_feed_records, one call
    per batch that holds no GIL): each reads its record's payload, checks the CRC, finds the PNG in the Example and inflates /
    unfilters it (zlib) straight into its frame of a batch buffer the caller may have pinned;
  * `prefetch` batches (config['data']['prefetch'], default max(2, cpu_thread_cnt / images per batch)) are decoded ahead of the
    consumer, several at a time, so that the pool is full at batch_size = 1 as well (the reference's default);
  * frames leave the host as uint8 -- the * (1/255) runs on the device (byolo_normalize_u8), bit-identical -- except through
    the plain iterator (`for imgs, names in dataset`), which yields the reference's float32 batches;
  * multi-GPU: a rank only reads, checks and decodes the records of ITS block of every global batch; the others are skipped by
    their framing (12 header bytes each)."""
import collections
import ctypes
import glob
import io
import os
import queue
import struct
import threading
import time

import numpy as np

from lib_yolo import model as _model

_MASK_DELTA = 0xA282EAD8


def _masked_crc(data):
    from byolo._lib import lib
    crc = lib.byolo_crc32c(data if isinstance(data, bytes) else bytes(data), len(data))     # (ctypes drops the GIL for the call)
    return ((((crc >> 15) | (crc << 17)) & 0xFFFFFFFF) + _MASK_DELTA) & 0xFFFFFFFF


def read_tfrecords(path, verify_crc=True):
    """Yield the payload bytes of every record in a TFRecord file."""
    size = os.path.getsize(path)
    with open(path, 'rb') as f:
        while True:
            head = f.read(12)
            if not head:
                return
            if len(head) < 12:
                raise IOError('truncated TFRecord header in {}'.format(path))
            length, = struct.unpack('<Q', head[:8])
            len_crc, = struct.unpack('<I', head[8:])
            if verify_crc and _masked_crc(head[:8]) != len_crc:
                raise IOError('corrupt TFRecord length CRC in {}'.format(path))
            if length > size - f.tell():              # a corrupt length must not turn into a giant read
                raise IOError('truncated TFRecord in {}'.format(path))
            data = f.read(length)
            tail = f.read(4)
            if len(data) < length or len(tail) < 4:
                raise IOError('truncated TFRecord in {}'.format(path))
            if verify_crc and _masked_crc(data) != struct.unpack('<I', tail)[0]:
                raise IOError('corrupt TFRecord data CRC in {}'.format(path))
            yield data


def write_tfrecords(path, payloads):
    """Inverse of read_tfrecords (test fixtures / small demo sets)."""
    with open(path, 'wb') as f:
        for data in payloads:
            head = struct.pack('<Q', len(data))
            f.write(head + struct.pack('<I', _masked_crc(head)) + data + struct.pack('<I', _masked_crc(data)))


# ---- minimal protobuf wire format (varint / length-delimited only) --------------------------------
def _varint(buf, pos):
    out = shift = 0
    while True:
        if pos >= len(buf) or shift > 63:
            raise ValueError('corrupt protobuf varint')
        b = buf[pos]
        pos += 1
        out |= (b & 0x7F) << shift
        if not b & 0x80:
            return out, pos
        shift += 7


def _fields(buf):
    pos, n = 0, len(buf)
    while pos < n:
        key, pos = _varint(buf, pos)
        num, wt = key >> 3, key & 7
        if wt == 0:
            val, pos = _varint(buf, pos)
        elif wt == 2:
            ln, pos = _varint(buf, pos)
            if ln > n - pos:
                raise ValueError('corrupt protobuf length')
            val = buf[pos:pos + ln]
            pos += ln
        elif wt == 1:
            val = buf[pos:pos + 8]
            pos += 8
        elif wt == 5:
            val = buf[pos:pos + 4]
            pos += 4
        else:
            raise ValueError('unsupported protobuf wire type {}'.format(wt))
        yield num, wt, val


def parse_example(data):
    """tf.train.Example -> {feature name: list of bytes / int / float values}.  Malformed input raises ValueError."""
    try:
        return _parse_example(memoryview(data))         # nested messages are slices of one buffer, not copies
    except (IndexError, TypeError, OverflowError, UnicodeDecodeError) as e:
        raise ValueError('corrupt tf.train.Example: {}'.format(e))


def _parse_example(data):
    out = {}
    for num, _, features in _fields(data):
        if num != 1:                                  # Example.features
            continue
        for fnum, _, entry in _fields(features):
            if fnum != 1:                             # Features.feature (map entry)
                continue
            name, feature = None, b''
            for k, _, v in _fields(entry):
                if k == 1:
                    name = bytes(v).decode('utf-8')
                elif k == 2:
                    feature = v
            vals = []
            for kind, _, lst in _fields(feature):     # 1 bytes_list, 2 float_list, 3 int64_list
                for vn, wt, v in _fields(lst):
                    if vn != 1:
                        continue
                    if kind == 1:
                        vals.append(bytes(v))
                    elif kind == 3:
                        if wt == 0:
                            vals.append(v - (1 << 64) if v >> 63 else v)
                        else:                         # packed
                            p = 0
                            while p < len(v):
                                x, p = _varint(v, p)
                                vals.append(x - (1 << 64) if x >> 63 else x)
                    elif kind == 2:
                        vals.extend(np.frombuffer(bytes(v), dtype='<f4').tolist())
            out[name] = vals
    return out


def _pb_bytes(num, payload):
    def vi(x):
        o = b''
        while True:
            b = x & 0x7F
            x >>= 7
            o += bytes([b | (0x80 if x else 0)])
            if not x:
                return o
    return vi((num << 3) | 2) + vi(len(payload)) + payload


def make_example(features):
    """{name: bytes | str | int} -> serialized tf.train.Example (fixtures / demos)."""
    def vi(x):
        x &= (1 << 64) - 1
        o = b''
        while True:
            b = x & 0x7F
            x >>= 7
            o += bytes([b | (0x80 if x else 0)])
            if not x:
                return o
    entries = b''
    for name, v in features.items():
        if isinstance(v, int):
            feat = _pb_bytes(3, vi((1 << 3) | 0) + vi(v))
        else:
            v = v.encode('utf-8') if isinstance(v, str) else v
            feat = _pb_bytes(1, _pb_bytes(1, v))
        entries += _pb_bytes(1, _pb_bytes(1, name.encode('utf-8')) + _pb_bytes(2, feat))
    return _pb_bytes(1, entries)




def decode_png_u8(encoded, shape):
    """`tf.image.decode_png(encoded, dtype=tf.uint8)` + `set_shape` of decode_img (`lib_yolo/dataset_utils.py:6-9`) for one
    record through the general decoder (Pillow): what the native pool falls back to for PNG flavours it does not read."""
    from PIL import Image
    img = np.asarray(Image.open(io.BytesIO(encoded)))
    if img.ndim == 2:
        img = img[:, :, None]
    if img.dtype != np.uint8:
        raise ValueError('only 8-bit PNGs are on this path (decode_png dtype=tf.uint8)')
    if tuple(img.shape) != tuple(shape):
        raise ValueError('image shape {} != config full_img_size {}'.format(img.shape, tuple(shape)))
    return img


def decode_img(encoded, shape):
    """`lib_yolo/dataset_utils.py:6-11`: decode PNG and scale to [0, 1] as float32."""
    return decode_png_u8(encoded, shape).astype(np.float32) * np.float32(1.0 / 255.0)      # convert_image_dtype(uint8 -> float32)


class _RecordFile:
    """Records of one TFRecord file by their framing only: (offset, length) of every payload; payloads are read on demand
    (os.pread: thread-safe), so a rank never touches the bytes of another rank's records."""

    def __init__(self, path, verify_crc):
        self.path, self.verify_crc = path, verify_crc
        self.fd = os.open(path, os.O_RDONLY)
        self.size = os.fstat(self.fd).st_size

    def __del__(self):
        try:
            os.close(self.fd)
        except Exception:
            pass

    def __iter__(self):
        pos = 0
        while pos < self.size:
            head = os.pread(self.fd, 12, pos)
            if len(head) < 12:
                raise IOError('truncated TFRecord header in {}'.format(self.path))
            length, = struct.unpack('<Q', head[:8])
            if self.verify_crc and _masked_crc(head[:8]) != struct.unpack('<I', head[8:])[0]:
                raise IOError('corrupt TFRecord length CRC in {}'.format(self.path))
            if length > self.size - pos - 16:         # a corrupt length must not turn into a giant read
                raise IOError('truncated TFRecord in {}'.format(self.path))
            yield (self, pos + 12, length)
            pos += 16 + length

    def payload(self, off, length):
        data = os.pread(self.fd, length + 4, off)
        if len(data) < length + 4:
            raise IOError('truncated TFRecord in {}'.format(self.path))
        if self.verify_crc and _masked_crc(data[:length]) != struct.unpack('<I', data[length:])[0]:
            raise IOError('corrupt TFRecord data CRC in {}'.format(self.path))
        return memoryview(data)[:length]


Shard = collections.namedtuple('Shard', 'u8 names lo n_global release error', defaults=(None,))
Shard.__doc__ = """One rank's block of one global batch: u8 [n_local,H,W,C] uint8 (a view of a batch buffer: call release() when
the frames have left it -- the buffer then goes back to the feeder), the block's file names, its offset `lo` in the global
batch (-> first_image: the dropout stream position) and the global batch's size.  `error` (iter_shards_u8(errors='yield')
only): the exception that reading / checking / decoding this rank's records of the batch raised -- the shard is then empty."""


class TestingDataset:
    """Iterable of (images [B,H,W,C] float32, [filenames]) batches; `placeholder` is what the model is
    built on.  `batch_size` is the GLOBAL batch, as in the reference (`lib_yolo/dataset_utils.py:188-219`).
    The entry points read it through `iter_shards_u8(rank, world)` (module docstring)."""
    __test__ = False

    def __init__(self, config, config_key='data'):
        self.__config = config
        info = config[config_key]
        self.files = sorted(glob.glob(info['file_pattern']))
        self.batch_size = config['batch_size']
        self.shape = tuple(config['full_img_size'])
        self.verify_crc = info.get('verify_crc', True)
        self.threads = max(1, int(config.get('cpu_thread_cnt', 1)))          # num_parallel_calls of the map stage (:196)
        # one process per GPU: N ranks x cpu_thread_cnt decode threads must fit the host (8 x 24 = 192 on a 256-thread node is fine,
        # 8 x 24 on a 64-thread one is not): at most the rank's share of the hardware threads (LOCAL_WORLD_SIZE: torchrun)
        local_world = max(1, int(os.environ.get('LOCAL_WORLD_SIZE', '1') or 1))
        self.threads = max(1, min(self.threads, (os.cpu_count() or 1) // local_world))
        self.prefetch = int(info.get('prefetch', 0))                         # batches decoded ahead (:199 prefetches 1); 0 = derive it (iter_shards_u8)
        self.placeholder = _model.Placeholder((self.batch_size,) + self.shape)

    def _records(self):
        # files.interleave(TFRecordDataset, cycle_length=2, block_length=1): record handles, no payload is read here
        pending = list(self.files)
        active = []
        while pending or active:
            while len(active) < 2 and pending:
                active.append(iter(_RecordFile(pending.pop(0), self.verify_crc)))
            for it in list(active):
                try:
                    yield next(it)
                except StopIteration:
                    active.remove(it)

    def _global_batches(self):
        recs = []
        for rec in self._records():
            recs.append(rec)
            if len(recs) == self.batch_size:
                yield recs
                recs = []
        if recs:                                       # last, smaller batch (tf.data batch keeps the remainder)
            yield recs

    @staticmethod
    def _filename(feats):
        names = feats.get('image/filename', [])
        return names[0].decode('utf-8') if names else ''

    def parse_example(self, example):
        feats = parse_example(example)
        return decode_img(feats['image/encoded'][0], self.shape), self._filename(feats)

    def _load_block(self, recs, buf, threads=None):
        """The map stage for the records of one block: payload (+ CRC) -> Example -> PNG decoded into buf[j] ([H,W,C] uint8), on
        `cpu_thread_cnt` native threads in ONE call that holds no GIL (byolo_feed_records); returns the file names."""
        from byolo import _lib
        n = len(recs)
        if n == 0:
            return []
        i32, i64 = ctypes.c_int32, ctypes.c_int64
        fds = (i32 * n)(*[r[0].fd for r in recs])
        offs = (i64 * n)(*[r[1] for r in recs])
        lens = (i64 * n)(*[r[2] for r in recs])
        status = (i32 * n)()
        found = (i32 * (3 * n))()
        cap = 1024
        names = ctypes.create_string_buffer(n * cap)
        h, w, c = self.shape
        assert buf.dtype == np.uint8 and buf.flags['C_CONTIGUOUS'] and buf.shape[0] >= n and tuple(buf.shape[1:]) == self.shape
        rc = _lib.lib.byolo_feed_records(fds, offs, lens, n, int(bool(self.verify_crc)), h, w, c, ctypes.c_void_p(buf.ctypes.data),
                                         int(threads or self.threads), names, cap, status, found)
        if rc < 0:
            raise ValueError('byolo_feed_records: bad argument (full_img_size {})'.format(self.shape))
        out = []
        for j, (rf, off, length) in enumerate(recs):
            st = status[j]
            if st == _lib.PNG_OK:
                out.append(names[j * cap:(j + 1) * cap].split(b'\0', 1)[0].decode('utf-8'))
                continue
            if st == _lib.FEED_IO:
                raise IOError('truncated TFRecord in {}'.format(rf.path))
            if st == _lib.FEED_CRC:
                raise IOError('corrupt TFRecord data CRC in {}'.format(rf.path))
            if st == _lib.PNG_SHAPE:
                raise ValueError('image shape {} != config full_img_size {}'.format(tuple(found[3 * j:3 * j + 3]), self.shape))
            # a malformed Example, or a PNG flavour the native decoder does not read (interlaced / palette / 16-bit) or finds
            # damaged: the general path decides (and raises what it always raised)
            feats = parse_example(rf.payload(off, length))
            enc = feats.get('image/encoded')
            if not enc:
                raise ValueError('record without image/encoded in {}'.format(rf.path))
            buf[j] = decode_png_u8(enc[0], self.shape)
            out.append(self._filename(feats))
        return out

    def __iter__(self):
        for sh in self.iter_shards_u8(0, 1):
            x = sh.u8.astype(np.float32) * np.float32(1.0 / 255.0)          # convert_image_dtype(uint8 -> float32)
            sh.release()
            yield x, sh.names

    def iter_shards_u8(self, rank, world, alloc=None, extra_buffers=2, errors='raise'):
        """Yields a `Shard` per global batch: the frames of this rank's contiguous block (byolo.dist.shard_range; may be empty
        for a last, short batch).  alloc(shape) -> uint8 ndarray provides the batch buffers (the driver passes pinned memory);
        `prefetch` + 1 + extra_buffers of them circulate: `prefetch` decoded or being decoded ahead of the consumer,
        extra_buffers with the consumer.

        The map stage runs `cpu_thread_cnt` decodes at a time whatever the batch size: up to `prefetch` batches are in the
        decode pool TOGETHER (each on min(cpu_thread_cnt, images of its block) native threads) and are handed over in order --
        at the reference's default batch_size = 1 (inference_epistemic.py:222) a 1024 x 1920 frame is 50 ms of inflate on one
        core, so one batch at a time would feed 20 img/s to a device that takes 41.  `prefetch` defaults to
        max(2, cpu_thread_cnt / images per block), at most 16.

        errors='raise': a record of this rank's block that cannot be read / checked / decoded raises here, at its batch's position.
        errors='yield': the batch arrives as an empty Shard carrying the exception (`error`) and the iteration goes on -- the
        multi-GPU driver needs that: the other ranks read only THEIR records and are about to enter the batch's collective, so
        this rank must take part in it (with a 'feed failed' status word) instead of leaving (byolo/inference.py)."""
        from concurrent.futures import ThreadPoolExecutor
        from byolo.dist import shard_range
        alloc = alloc or (lambda shape: np.empty(shape, dtype=np.uint8))
        cap = max(1, shard_range(self.batch_size, 0, world)[1])              # the largest block of a full batch
        prefetch = self.prefetch if self.prefetch > 0 else max(2, min(16, -(-self.threads // cap)))
        # `prefetch` calls decode at once: each gets its share of cpu_thread_cnt (a block of 64 images used to start 2 x 24 threads)
        # (a LOCAL of this iterator: two iterators of one dataset -- another world, another prefetch -- keep their own)
        per_call = max(1, -(-self.threads // prefetch))
        free = queue.Queue()
        for _ in range(prefetch + 1 + max(1, extra_buffers)):
            free.put(alloc((cap,) + self.shape))
        ready = queue.Queue(maxsize=prefetch)                                # futures, in batch order
        stop = threading.Event()

        def put(item):
            while not stop.is_set():
                try:
                    ready.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    pass
            return False

        def load(recs, buf, lo, n_glob):
            try:
                return buf, len(recs), self._load_block(recs, buf, threads=per_call), lo, n_glob
            except Exception as e:                                           # a failed record reaches the consumer in order
                return buf, 0, e, lo, n_glob

        def feeder():
            pool = ThreadPoolExecutor(max_workers=prefetch, thread_name_prefix='byolo-feed')
            try:
                for recs in self._global_batches():
                    lo, hi = shard_range(len(recs), rank, world)
                    buf = None
                    while buf is None:
                        if stop.is_set():
                            return
                        try:
                            buf = free.get(timeout=0.1)
                        except queue.Empty:
                            pass
                    if not put(pool.submit(load, recs[lo:hi], buf, lo, len(recs))):
                        return
                put(None)
            except BaseException as e:                                        # (the record index itself: framing errors) delivered in order
                put(e)
            finally:
                pool.shutdown(wait=True)

        th = threading.Thread(target=feeder, name='byolo-feeder', daemon=True)
        th.start()
        try:
            while True:
                item = ready.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                buf, n, names, lo, n_glob = item.result()
                if isinstance(names, Exception):
                    if errors != 'yield':
                        raise names
                    yield Shard(buf[:0], [], lo, n_glob, (lambda b=buf: free.put(b)), names)
                    continue
                yield Shard(buf[:n], names, lo, n_glob, (lambda b=buf: free.put(b)))
        finally:
            stop.set()
            th.join(timeout=10)


# =============================================================================================================================
# Training / validation feed -- mirror of make_parse_fn / create_dataset / TrainValDataset (lib_yolo/dataset_utils.py:14-156)
# =============================================================================================================================
#
# Record stream of a split (create_dataset + the shuffle / repeat of TrainValDataset): the files of the glob, shuffled with a
# buffer of num_shards -> interleave(cycle_length=2, block_length=1) -> shuffle with tf.data's buffer algorithm (fill the buffer,
# emit a uniform pick, refill) -> the next epoch reshuffles -> repeat.  What is shuffled are record REFERENCES (file, offset,
# length), not decoded frames: the augmentation draws are keyed by the record's position in its epoch (byolo/augment.py), so
# the distribution of batches is the same, and a buffer of 2000 decoded 1024 x 1920 frames (about 26 GB) is never held.
# Shuffles draw from generators keyed by (config['seed'], split, epoch), so a run is reproducible; the stream restarts from its
# seed when a training run resumes (as the reference's one-shot iterator does).
#
# Per batch (TrainValDataset): payloads (cache: True keeps them in host memory after the first read) -> tf.train.Example ->
# boxes / labels (numpy) and the PNG, decoded on cpu_thread_cnt native threads (byolo_png_decode_batch) into a pinned uint8
# batch buffer; `prefetch` batches (default: max(2, cpu_thread_cnt / batch_size), at most 16) are prepared ahead.  The consumer
# copies each image's row band [y0, y0 + ch) to the device on a side stream and runs ONE byolo_augment_batch launch on its own stream after an event, so the crop, resize,
# flip, blur, colour and noise of the whole batch are one kernel; the next batch's copy is started before the batch is returned.
_TRAIN_KEYS = ('image/encoded', 'image/object/bbox/ymin', 'image/object/bbox/xmin', 'image/object/bbox/ymax', 'image/object/bbox/xmax',
               'image/object/class/label')


def make_parse_fn(config):
    """parse_example of lib_yolo/dataset_utils.py:14-53: record payload -> (PNG bytes, boxes [n, 4] float32 as (ymin, xmin, ymax,
    xmax), labels [n] int32, shifted by -1 when implicit_background_class)."""
    shift = 1 if config['implicit_background_class'] else 0

    def parse(example):
        feats = parse_example(example)
        enc = feats.get('image/encoded')
        if not enc:
            raise ValueError('record without image/encoded')
        cols = [np.asarray(feats.get(k, []), dtype=np.float32) for k in _TRAIN_KEYS[1:5]]
        n = max(len(c) for c in cols)
        cols = [np.pad(c, (0, n - len(c))) for c in cols]                  # sparse_tensor_to_dense(default_value=0)
        boxes = np.stack(cols, axis=1).astype(np.float32) if n else np.zeros((0, 4), np.float32)
        labels = np.asarray(feats.get('image/object/class/label', []), dtype=np.int64).astype(np.int32) - shift
        return enc[0], boxes, labels

    return parse


def make_train_example(png, boxes, labels, filename=''):
    """A training record as create_tf_records_citypersons.py writes one: image/encoded, image/height / width, the box
    coordinates as float lists and the class labels as an int64 list (fixtures / demo shards)."""
    import struct

    def vi(x):
        x &= (1 << 64) - 1
        o = b''
        while True:
            b = x & 0x7F
            x >>= 7
            o += bytes([b | (0x80 if x else 0)])
            if not x:
                return o
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    feats = {'image/encoded': _pb_bytes(1, _pb_bytes(1, png)), 'image/filename': _pb_bytes(1, _pb_bytes(1, filename.encode('utf-8'))),
             'image/object/class/label': _pb_bytes(3, _pb_bytes(1, b''.join(vi(int(v)) for v in np.asarray(labels).reshape(-1))))}
    for k, name in enumerate(('ymin', 'xmin', 'ymax', 'xmax')):
        feats['image/object/bbox/' + name] = _pb_bytes(2, _pb_bytes(1, struct.pack('<%df' % len(boxes), *boxes[:, k])))
    entries = b''.join(_pb_bytes(1, _pb_bytes(1, n.encode('utf-8')) + _pb_bytes(2, f)) for n, f in feats.items())
    return _pb_bytes(1, entries)


def shuffle_buffer(items, buffer_size, rng):
    """tf.data shuffle: fill a buffer of buffer_size, emit a uniform pick, refill it from the input."""
    it = iter(items)
    buf = []
    for x in it:
        buf.append(x)
        if len(buf) >= max(1, int(buffer_size)):
            break
    while buf:
        i = int(rng.integers(len(buf)))
        out = buf[i]
        buf[i] = buf[-1]
        buf.pop()
        for x in it:
            buf.append(x)
            break
        yield out


class RecordStream:
    """The record stream of one split (config[dataset_key]): `epoch(e)` = the record references of epoch e in stream order,
    iterating yields (epoch, position in the epoch, reference) forever (repeat)."""

    def __init__(self, config, dataset_key, split=None):
        info = config[dataset_key]
        self.split = split or dataset_key
        self.seed = int(config.get('seed', 0))
        self.files = sorted(glob.glob(info['file_pattern']))
        if not self.files:
            raise FileNotFoundError('no TFRecord file matches {}'.format(info['file_pattern']))
        self.num_shards = int(info.get('num_shards', 1))
        self.buffer_size = int(info.get('shuffle_buffer_size', 1))
        self.cache = bool(info.get('cache', False))
        self.verify_crc = info.get('verify_crc', True)
        self._rf = {}
        self._recs = {}
        self._payloads = {}

    def _rng(self, epoch, purpose):
        from byolo.augment import SPLITS
        return np.random.default_rng([self.seed & (2 ** 63 - 1), SPLITS[self.split], int(epoch), 0, purpose])

    def records(self, path):
        if path not in self._recs:
            self._rf[path] = _RecordFile(path, self.verify_crc)
            self._recs[path] = [(off, ln) for _, off, ln in self._rf[path]]
        return self._recs[path]

    def epoch(self, e):
        if self.split == 'eval':                  # the files in sorted order, their records in file order: no shuffle
            return ((p, k) for p in self.files for k in range(len(self.records(p))))
        files = list(shuffle_buffer(self.files, self.num_shards, self._rng(e, 1)))

        def interleaved():                        # interleave(TFRecordDataset, cycle_length=2, block_length=1)
            pending, active = list(files), []
            while pending or active:
                while len(active) < 2 and pending:
                    p = pending.pop(0)
                    active.append(iter([(p, k) for k in range(len(self.records(p)))]))
                for a in list(active):
                    try:
                        yield next(a)
                    except StopIteration:
                        active.remove(a)
        return shuffle_buffer(interleaved(), self.buffer_size, self._rng(e, 2))

    def __iter__(self):
        e = 0
        while True:
            for pos, ref in enumerate(self.epoch(e)):
                yield e, pos, ref
            if self.split == 'eval':              # one pass
                return
            e += 1

    def payload(self, ref):
        if ref in self._payloads:
            return self._payloads[ref]
        path, k = ref
        off, ln = self.records(path)[k]
        data = bytes(self._rf[path].payload(off, ln))
        if self.cache:
            self._payloads[ref] = data
        return data


def create_dataset(config, dataset_key):
    """create_dataset of lib_yolo/dataset_utils.py:103-117, as a record stream (the parse stage runs in TrainValDataset)."""
    return RecordStream(config, dataset_key)


class _HostBatch:
    __slots__ = ('buf', 'plans', 'boxes', 'labels', 'counts', 'keys', 'error')


class _Feed:
    """One split's batches (the iterator of TrainValDataset.train / .val)."""

    def __init__(self, config, dataset_key, split, device=None):
        import torch
        from byolo import augment
        self._augment = augment
        self.config = config
        self.split = split
        self.stream = RecordStream(config, dataset_key, split)
        self.parse = make_parse_fn(config)
        self.B = int(config['batch_size'])
        self.full = tuple(int(v) for v in config['full_img_size'][:2])
        self.out_hw = tuple(int(v) for v in (config['crop_img_size'] if config['crop'] else config['full_img_size'])[:2])
        self.threads = max(1, int(config.get('cpu_thread_cnt', 1)))
        # batches prepared ahead, each decoded on its share of cpu_thread_cnt: enough of them that every thread has an image
        self.prefetch = max(2, int(config[dataset_key].get('prefetch', 0)) or min(16, -(-self.threads // self.B)))
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        Hf, Wf = self.full
        self._free = queue.Queue()
        for _ in range(self.prefetch + 2):
            self._free.put(torch.empty((self.B, Hf, Wf, 3), dtype=torch.uint8, pin_memory=True))
        self._dev = [torch.empty((self.B, Hf, Wf, 3), dtype=torch.uint8, device=self.device) for _ in range(2)]
        self._dev_free = [None, None]                     # event after the last augment that read the slot
        self._slot = 0
        self._side = torch.cuda.Stream(self.device)
        self._pending = None                              # (host batch, device slot, copy event)
        self._done = False                                # split 'eval': the stream has ended
        self.host_seconds = {'augment': 0.0, 'copy': 0.0}  # host time of next(): event wait + augment launch / issuing copies
        self._returning = []
        self._ready = queue.Queue(maxsize=self.prefetch)
        self._stop = threading.Event()
        self._th = threading.Thread(target=self._producer, name='byolo-train-feed-%s' % split, daemon=True)
        self._th.start()

    # ---- host side ---------------------------------------------------------------------------------------------------
    def _load(self, items, buf, threads):
        from byolo import hostio, _lib
        hb = _HostBatch()
        hb.buf, hb.error = buf, None
        try:
            aug = self._augment
            n = len(items)
            plans = aug.empty_plans(n)
            encs, boxes, labels, keys = [], [], [], []
            for k, (e, pos, ref) in enumerate(items):
                try:
                    enc, bx, lb = self.parse(self.stream.payload(ref))
                except ValueError as err:
                    raise ValueError('{} record {}: {}'.format(ref[0], ref[1], err))
                win = aug.draw(self.config, self.split, e, pos, plans[k])
                bx, lb = aug.apply_to_boxes(plans[k], win, bx, lb)
                encs.append(enc)
                boxes.append(bx)
                labels.append(lb)
                keys.append(ref)
            arr = buf.numpy()
            _, status, found = hostio.decode_png_batch(encs, self.full + (3,), out=arr, threads=threads)
            for k in range(n):
                if status[k] == _lib.PNG_OK:
                    continue
                if status[k] == _lib.PNG_SHAPE:
                    raise ValueError('{} record {}: image shape {} != config full_img_size {}'.format(
                        keys[k][0], keys[k][1], tuple(int(v) for v in found[k]), tuple(self.config['full_img_size'])))
                try:
                    arr[k] = decode_png_u8(encs[k], self.full + (3,))
                except Exception as err:
                    raise ValueError('{} record {}: {}'.format(keys[k][0], keys[k][1], err))
            plans['row0'] = plans['y0']
            nmax = max([1] + [len(b) for b in boxes])
            hb.boxes = np.zeros((n, nmax, 4), np.float32)
            hb.labels = np.zeros((n, nmax), np.int32)
            hb.counts = np.array([len(b) for b in boxes], np.int32)
            for k in range(n):
                hb.boxes[k, :len(boxes[k])] = boxes[k]
                hb.labels[k, :len(labels[k])] = labels[k]
            hb.plans, hb.keys = plans, keys
        except Exception as err:
            hb.error = err
        return hb

    def _producer(self):
        from concurrent.futures import ThreadPoolExecutor
        per_call = max(1, -(-self.threads // self.prefetch))
        pool = ThreadPoolExecutor(max_workers=self.prefetch, thread_name_prefix='byolo-train-decode')
        try:
            items = []
            for item in self.stream:
                items.append(item)
                if len(items) < self.B:
                    continue
                buf = None
                while buf is None:
                    if self._stop.is_set():
                        return
                    try:
                        buf = self._free.get(timeout=0.1)
                    except queue.Empty:
                        pass
                fut = pool.submit(self._load, items, buf, per_call)
                items = []
                while not self._stop.is_set():
                    try:
                        self._ready.put(fut, timeout=0.1)
                        break
                    except queue.Full:
                        pass
                if self._stop.is_set():
                    return
            if self.split == 'eval':                     # one pass: the last short batch is kept, then the stream ends
                tail = []
                while items and not tail and not self._stop.is_set():
                    try:
                        tail = [pool.submit(self._load, items, self._free.get(timeout=0.1), per_call)]
                    except queue.Empty:
                        pass
                for item in tail + [StopIteration()]:
                    while not self._stop.is_set():
                        try:
                            self._ready.put(item, timeout=0.1)
                            break
                        except queue.Full:
                            pass
        except BaseException as err:                     # framing errors reach the consumer in order
            self._ready.put(err)
        finally:
            pool.shutdown(wait=True)

    # ---- device side -------------------------------------------------------------------------------------------------
    def _start_copy(self, block):
        import torch
        try:
            item = self._ready.get(block=block)
        except queue.Empty:
            return
        if isinstance(item, StopIteration):              # the 'eval' split's one pass is over
            self._done = True
            return
        if isinstance(item, BaseException):
            raise item
        hb = item.result()
        if hb.error is not None:
            self._free.put(hb.buf)
            raise hb.error
        slot = self._slot
        self._slot ^= 1
        dev = self._dev[slot]
        with torch.cuda.stream(self._side):
            if self._dev_free[slot] is not None:
                self._side.wait_event(self._dev_free[slot])
            for k in range(len(hb.plans)):
                y0, ch = int(hb.plans[k]['y0']), int(hb.plans[k]['ch'])
                dev[k, :ch].copy_(hb.buf[k, y0:y0 + ch], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._side)
        self._pending = (hb, slot, ev)

    def __iter__(self):
        return self

    def __next__(self):
        import torch
        for buf, ev in self._returning:                  # pinned buffers whose copies are done go back to the producer
            ev.synchronize()
            self._free.put(buf)
        self._returning = []
        if self._pending is None and not self._done:
            self._start_copy(block=True)
        if self._pending is None:
            raise StopIteration
        hb, slot, ev = self._pending
        self._pending = None
        t0 = time.perf_counter()
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        src_h = max(1, int(hb.plans['ch'].max()))
        plans = hb.plans.copy()
        plans['row0'] = plans['y0']
        dev = self._dev[slot][:len(plans), :src_h]
        img = self._augment.augment_batch(dev, plans, self.out_hw, stream=cur.cuda_stream)
        done = torch.cuda.Event()
        done.record(cur)
        t1 = time.perf_counter()
        self._dev_free[slot] = done
        self._returning.append((hb.buf, ev))
        if not self._done:
            self._start_copy(block=False)                # the next batch's copy overlaps the caller's step
        self.host_seconds['augment'] += t1 - t0
        self.host_seconds['copy'] += time.perf_counter() - t1
        plans['row0'] = 0
        return {'img': img, 'boxes': hb.boxes, 'labels': hb.labels, 'counts': hb.counts, 'plans': plans, 'keys': hb.keys}

    def close(self):
        import torch
        self._side.synchronize()                         # no copy into the device slots may outlive the feed
        torch.cuda.current_stream(self.device).synchronize()
        self._stop.set()
        try:
            while True:
                self._ready.get_nowait()
        except queue.Empty:
            pass
        self._th.join(timeout=10)


class TrainValDataset:
    """TrainValDataset of lib_yolo/dataset_utils.py:120-167: `train` and `val` iterate batches {'img': float32 CUDA tensor
    [B, h, w, 3] on the current stream, 'boxes' [B, nmax, 4], 'labels' [B, nmax], 'counts' [B] (numpy), 'plans' (the batch's
    byolo.augment plans, frame coordinates), 'keys' [(file, record index)]}.  Train: crop -> augment; val: the same random crop,
    no augmentation.  The ground truth is encoded on the device by the trainer (byolo_encode_gt), so the blueprint is only
    checked for its shape."""

    def __init__(self, model_blueprint, config):
        if config['crop']:
            from lib_yolo.data_augmentation import ImageCropper
            ImageCropper(config)                          # the aspect-ratio assertion
        self.blueprint = model_blueprint
        self.train = _Feed(config, 'train', 'train')
        self.val = _Feed(config, 'val', 'val')

    def close(self):
        self.train.close()
        self.val.close()
