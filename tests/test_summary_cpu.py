"""CPU: the TensorBoard event files of the two training modes (kpx_amd.summary), decoded independently of the writer -- a pure-Python
CRC-32C checks every record frame, google.protobuf parses Event / Summary from a descriptor built here from the published field numbers
of event.proto and summary.proto, PIL decodes the PNGs -- plus the numpy restatement of TF 1.12's NormalizeFloatImage that the GPU tests
hold the HIP conversion to, and the argument checks of the ABI-7 entries."""
import io
import os
import re
import socket
import struct

import numpy as np
import pytest
import torch

# ------------------------------------------------------------------------------------------------ independent decoder
_CRC_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0x82F63B78 if _c & 1 else _c >> 1
    _CRC_TABLE.append(_c)


def crc32c_py(data):
    crc = 0xffffffff
    for b in data:
        crc = _CRC_TABLE[(crc ^ b) & 0xff] ^ (crc >> 8)
    return crc ^ 0xffffffff


def masked_py(data):
    crc = crc32c_py(data)
    return (((crc >> 15) | (crc << 17)) + 0xa282ead8) & 0xffffffff


def records_py(path):
    buf = open(path, 'rb').read()
    pos, out = 0, []
    while pos < len(buf):
        length = buf[pos:pos + 8]
        n = struct.unpack('<Q', length)[0]
        assert struct.unpack('<I', buf[pos + 8:pos + 12])[0] == masked_py(length)
        data = buf[pos + 12:pos + 12 + n]
        assert len(data) == n
        assert struct.unpack('<I', buf[pos + 12 + n:pos + 16 + n])[0] == masked_py(data)
        out.append(data)
        pos += 16 + n
    return out


_CLASSES = {}


def proto_classes():
    """Event / Summary message classes from the published field numbers (tensorflow/core/util/event.proto, framework/summary.proto)."""
    if _CLASSES:
        return _CLASSES
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fdp = descriptor_pb2.FileDescriptorProto(name='kpx_test_event.proto', package='kpxtest', syntax='proto3')

    def field(msg, name, number, ftype, label=F.LABEL_OPTIONAL, type_name=None):
        f = msg.field.add(name=name, number=number, type=ftype, label=label)
        if type_name:
            f.type_name = type_name

    summ = fdp.message_type.add(name='Summary')
    img = summ.nested_type.add(name='Image')
    field(img, 'height', 1, F.TYPE_INT32)
    field(img, 'width', 2, F.TYPE_INT32)
    field(img, 'colorspace', 3, F.TYPE_INT32)
    field(img, 'encoded_image_string', 4, F.TYPE_BYTES)
    val = summ.nested_type.add(name='Value')
    field(val, 'node_name', 7, F.TYPE_STRING)
    field(val, 'tag', 1, F.TYPE_STRING)
    field(val, 'simple_value', 2, F.TYPE_FLOAT)
    field(val, 'image', 4, F.TYPE_MESSAGE, type_name='.kpxtest.Summary.Image')
    field(summ, 'value', 1, F.TYPE_MESSAGE, F.LABEL_REPEATED, '.kpxtest.Summary.Value')
    ev = fdp.message_type.add(name='Event')
    field(ev, 'wall_time', 1, F.TYPE_DOUBLE)
    field(ev, 'step', 2, F.TYPE_INT64)
    field(ev, 'file_version', 3, F.TYPE_STRING)
    field(ev, 'graph_def', 4, F.TYPE_BYTES)
    field(ev, 'summary', 5, F.TYPE_MESSAGE, type_name='.kpxtest.Summary')
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    for name in ('Event', 'Summary'):
        _CLASSES[name] = message_factory.GetMessageClass(pool.FindMessageTypeByName('kpxtest.' + name))
    return _CLASSES


def events_py(path):
    """-> list of Event messages (every frame checked)."""
    Event = proto_classes()['Event']
    out = []
    for data in records_py(path):
        e = Event()
        e.ParseFromString(data)
        out.append(e)
    return out


def decode_png(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


def event_sets(path):
    """[(step, [tags])] of every Event after the file-version header."""
    evs = events_py(path)
    assert evs[0].file_version == 'brain.Event:2' and evs[0].wall_time > 0 and not evs[0].HasField('summary')
    return [(e.step, [v.tag for v in e.summary.value]) for e in evs[1:]]


def event_file(logdir):
    files = [f for f in os.listdir(logdir) if f.startswith('events.out.tfevents.')]
    assert len(files) == 1, files
    assert re.fullmatch(r'events\.out\.tfevents\.\d{10}\.' + re.escape(socket.gethostname()), files[0]), files[0]
    return os.path.join(logdir, files[0])


# ------------------------------------------------------------------------------------------------ numpy restatement (TF 1.12)
PREMAPS = ('identity', 'x255', 'unit255', 'unit255_clip')


def premap_np(x, premap):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        if premap == 'x255':
            return x * np.float32(255)
        if premap in ('unit255', 'unit255_clip'):
            v = (x + np.float32(1)) / np.float32(2) * np.float32(255)
            if premap == 'unit255_clip':
                v = np.where(np.float32(255) < v, np.float32(255), v)      # minimum(t, 255): std::min keeps a NaN first operand
                v = np.where(v < np.float32(0), np.float32(0), v)          # maximum(., 0)
            return v.astype(np.float32)
    return x


def normalize_float_image(v):
    """SummaryImageOp::NormalizeFloatImage on one pre-mapped image [H,W,C] fp32 -> uint8."""
    v = np.asarray(v, np.float32)
    c = v.shape[-1]
    finite = np.isfinite(v).all(axis=-1)
    vals = v[finite]
    mn = np.float32(vals.min()) if vals.size else np.float32(np.inf)
    mx = np.float32(vals.max()) if vals.size else np.float32(-np.inf)
    if mn < 0:
        m = max(abs(mn), abs(mx))
        scale = np.float32(0) if m < np.float32(1e-6) else np.float32(np.float32(127) / np.float32(m))
        offset = np.float32(128)
    else:
        scale = np.float32(0) if mx < np.float32(1e-6) else np.float32(np.float32(255) / mx)
        offset = np.float32(0)
    out = np.empty(v.shape, np.uint8)
    with np.errstate(invalid='ignore', over='ignore'):
        aff = (v * scale).astype(np.float32) + offset                       # two roundings, as Eigen evaluates x * scale + offset
    out[finite] = np.trunc(aff[finite]).astype(np.uint8)
    out[~finite] = np.array([255, 0, 0, 255], np.uint8)[:c]
    return out


def summary_image_np(x, premap, max_outputs=2):
    x = np.asarray(x, np.float32)[:max_outputs]
    return np.stack([normalize_float_image(premap_np(img, premap)) for img in x])


# ------------------------------------------------------------------------------------------------ tests: the restatement
def test_restatement_positive_branch_scales_max_to_255():
    img = np.array([[[0.0], [1.0], [2.0], [4.0]]], np.float32)              # [1,4,1]
    assert normalize_float_image(img).ravel().tolist() == [0, 63, 127, 255]
    # an image already in [0, 255] is still rescaled so that its maximum becomes 255
    assert normalize_float_image(np.array([[[10.0], [100.0]]], np.float32)).ravel().tolist() == [25, 255]


def test_restatement_negative_branch_centres_on_128():
    img = np.array([[[-2.0], [0.0], [1.0]]], np.float32)
    # scale = 127 / 2: -2 -> 1, 0 -> 128, 1 -> 191.5 -> 191
    assert normalize_float_image(img).ravel().tolist() == [1, 128, 191]


def test_restatement_zero_threshold():
    tiny = np.array([[[0.0], [9e-7]]], np.float32)
    assert normalize_float_image(tiny).ravel().tolist() == [0, 0]            # max below 1e-6: scale 0
    tiny_neg = np.array([[[-9e-7], [5e-7]]], np.float32)
    assert normalize_float_image(tiny_neg).ravel().tolist() == [128, 128]    # max(|min|, |max|) below 1e-6: scale 0, offset 128
    above = np.array([[[0.0], [2e-6]]], np.float32)
    assert normalize_float_image(above).ravel().tolist() == [0, 255]


def test_restatement_non_finite_pixels_get_the_bad_colour_and_are_ignored_by_min_max():
    img = np.array([[[1.0, 2.0, 4.0], [np.nan, 0.0, 0.0], [100.0, np.inf, 1.0], [-50.0, 0.0, 0.0]]], np.float32)
    out = normalize_float_image(img)
    assert out[0, 1].tolist() == [255, 0, 0] and out[0, 2].tolist() == [255, 0, 0]
    # min -50 over the finite pixels (the 100 of the inf pixel is not counted): scale = 127 / 50
    assert out[0, 3].tolist() == [1, 128, 128]
    assert normalize_float_image(np.full((1, 2, 4), np.nan, np.float32)).reshape(-1, 4).tolist() == [[255, 0, 0, 255]] * 2
    assert normalize_float_image(np.full((1, 1, 1), np.inf, np.float32)).ravel().tolist() == [255]


def test_restatement_clip_keeps_nan_and_clips_inf():
    x = np.array([np.nan, np.inf, -np.inf, 3.0, -3.0, 0.0], np.float32)
    v = premap_np(x, 'unit255_clip')
    assert np.isnan(v[0]) and v[1:].tolist() == [255.0, 0.0, 255.0, 0.0, 127.5]
    v = premap_np(x, 'unit255')
    assert np.isnan(v[0]) and np.isposinf(v[1]) and np.isneginf(v[2])


# ------------------------------------------------------------------------------------------------ tests: PNG, records, reader
@pytest.mark.parametrize('shape', [(5, 7, 1), (4, 9, 3), (3, 1, 3), (2, 3, 4), (1, 13, 1)])
def test_png_round_trips_through_pil(shape):
    from kpx_amd import summary
    img = np.random.RandomState(sum(shape)).randint(0, 256, size=shape).astype(np.uint8)
    got = decode_png(summary.encode_png(img))
    assert np.array_equal(got.reshape(shape), img)


def test_writer_frames_header_and_values_decode_independently(tmp_path):
    from kpx_amd import summary
    w = summary.EventFileWriter(str(tmp_path / 'train'))
    imgs = np.random.RandomState(0).randint(0, 256, size=(3, 6, 5, 3)).astype(np.uint8)
    mask = np.random.RandomState(1).randint(0, 256, size=(1, 4, 7, 1)).astype(np.uint8)
    w.add_summary([summary.scalar_value('D_real', 0.25), summary.scalar_value('D_fake', -1.5e-3)], 0)
    w.add_summary(summary.image_values('im', imgs, max_outputs=2) + summary.image_values('mask', mask, max_outputs=2), 7)
    w.add_summary([summary.scalar_value('lr', np.float32(1e-4))], 2 ** 40)
    w.close()
    path = event_file(str(tmp_path / 'train'))
    assert event_sets(path) == [(0, ['D_real', 'D_fake']), (7, ['im/image/0', 'im/image/1', 'mask/image/0']), (2 ** 40, ['lr'])]
    evs = events_py(path)
    assert evs[1].summary.value[0].simple_value == 0.25
    assert evs[1].summary.value[1].simple_value == np.float32(-1.5e-3)
    assert evs[3].summary.value[0].simple_value == np.float32(1e-4)
    for v, want in zip(evs[2].summary.value, [imgs[0], imgs[1], mask[0]]):
        assert (v.image.height, v.image.width, v.image.colorspace) == want.shape
        assert np.array_equal(decode_png(v.image.encoded_image_string).reshape(want.shape), want)
    # max_outputs = 1: the tag has no index
    assert summary.image_values('x', imgs, max_outputs=1)[0] == summary.image_values('x', imgs[:1], max_outputs=1)[0]
    # the package's reader agrees with the independent decoder
    mine = summary.read_events(path)
    assert len(mine) == len(evs)
    assert mine[0]['file_version'] == 'brain.Event:2'
    for a, b in zip(mine, evs):
        assert a['wall_time'] == b.wall_time and a['step'] == b.step
        assert [v['tag'] for v in a['values']] == [v.tag for v in b.summary.value]
        for va, vb in zip(a['values'], b.summary.value):
            if 'simple_value' in va:
                assert va['simple_value'] == vb.simple_value
            else:
                assert va['image']['encoded_image_string'] == vb.image.encoded_image_string
    assert summary.scalars(path) == {'D_real': [(0, 0.25)], 'D_fake': [(0, float(np.float32(-1.5e-3)))], 'lr': [(2 ** 40, float(np.float32(1e-4)))]}


def test_reader_rejects_a_corrupted_record(tmp_path):
    from kpx_amd import summary
    w = summary.EventFileWriter(str(tmp_path))
    w.add_summary([summary.scalar_value('a', 1.0)], 1)
    w.close()
    path = event_file(str(tmp_path))
    buf = bytearray(open(path, 'rb').read())
    buf[-6] ^= 1
    open(path, 'wb').write(bytes(buf))
    with pytest.raises(ValueError):
        summary.read_events(path)


# ------------------------------------------------------------------------------------------------ tests: the models' event sets
def _cfg(tmp_path, k=5):
    return {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': 2},
            'model': {'n_pts': k, 'n_action': 3, 'cell_info': [8, 8], 'vae_dim': 4},
            'paths': {'log_dir': str(tmp_path), 'vggnet': None}}


@pytest.fixture
def cpu_image_ops(monkeypatch):
    """The GPU pieces of a summary replaced by CPU stand-ins (the numpy restatement; key-point renders of the right shape), so the
    event sets the models write can be checked here; the GPU tests run the real kernels."""
    from kpx_amd import model_utils, ops
    monkeypatch.setattr(ops, 'summary_image_u8', lambda x, premap, max_outputs=2: torch.from_numpy(summary_image_np(x.numpy(), premap, max_outputs)))
    monkeypatch.setattr(model_utils, 'render_point_maps', lambda mu, hw, colors, inv_std=14.3: torch.rand(mu.shape[0], hw[0], hw[1], 3))
    monkeypatch.setattr(ops, 'point_seq_strip_rgb', lambda mu, h, w, colors, recolour=True, inv_std=14.3, max_outputs=None:
                        torch.rand(min(mu.shape[0], max_outputs), h, mu.shape[1] * w, 3))


def _detector_last(b, r, k):
    rs = np.random.RandomState(3)
    t = lambda *s: torch.from_numpy(rs.uniform(-1, 1, size=s).astype(np.float32))
    return dict(d_losses=torch.tensor([1.5, 0.75, 0.75]), recon=torch.tensor([3.0]), adv=torch.tensor([0.5, 0.5, 0.0]), lr=float(np.float32(1e-4)),
                fwd=dict(final_output=t(b, r, r, 3), crude_output=t(b, r, r, 3) * 2, mask=(t(b, r, r, 1) + 1) / 2, current_points=t(b, k, 2),
                         future_points=t(b, k, 2)))


def test_detector_translator_train_and_test_event_sets(tmp_path, cpu_image_ops, monkeypatch):
    from kpx_amd.detector_translator_model import DetectorTranslatorModel
    b, r, k = 3, 16, 5
    model = DetectorTranslatorModel(_cfg(tmp_path, k), device='cpu', image_size=r)
    model.initialize_loggers(str(tmp_path))
    last = _detector_last(b, r, k)
    monkeypatch.setattr(model, '_graph_eligible', lambda feed: False)
    monkeypatch.setattr(model, '_train_step_eager', lambda feed: setattr(model, 'last', last))
    feed = {'image': torch.rand(b, r, r, 3) * 2 - 1, 'future_image': torch.rand(b, r, r, 3) * 2 - 1}
    model.train_step(None, feed, 5, b, should_write_summary=True)
    model.train_step(None, feed, 6, b, should_write_summary=False)
    model.close_loggers()
    imgs = ['future_im', 'im', 'current_points', 'future_points', 'future_im_crude', 'future_im_pred', 'mask']
    img_tags = ['%s/image/%d' % (n, i) for n in imgs for i in range(2)]
    path = event_file(str(tmp_path / 'detector_translator' / 'train'))
    assert event_sets(path) == [(5, ['D_real', 'D_fake']), (5, ['reconstruction_metric', 'G_adv_loss']), (5, img_tags), (5, ['lr'])]
    evs = events_py(path)
    assert [v.simple_value for v in evs[1].summary.value] == [0.75, 0.75]
    assert [v.simple_value for v in evs[2].summary.value] == [3.0, 0.5]
    assert evs[4].summary.value[0].simple_value == np.float32(1e-4)
    byname = {v.tag: v.image for v in evs[3].summary.value}
    assert byname['mask/image/1'].colorspace == 1 and byname['im/image/0'].colorspace == 3
    want = summary_image_np(last['fwd']['final_output'].numpy(), 'unit255_clip')[1]
    assert np.array_equal(decode_png(byname['future_im_pred/image/1'].encoded_image_string), want)
    want = summary_image_np(feed['future_image'].numpy(), 'unit255')[0]
    assert np.array_equal(decode_png(byname['future_im/image/0'].encoded_image_string), want)
    assert event_sets(event_file(str(tmp_path / 'detector_translator' / 'test'))) == []


def test_detector_translator_test_step_event_set(tmp_path, cpu_image_ops, monkeypatch):
    from kpx_amd.detector_translator_model import DetectorTranslatorModel
    b, r, k = 1, 16, 5
    model = DetectorTranslatorModel(_cfg(tmp_path, k), device='cpu', image_size=r)
    model.initialize_loggers(str(tmp_path))
    last = _detector_last(b, r, k)
    monkeypatch.setattr(model, '_define_forward_pass', lambda im, fut, update_moving=True: last['fwd'])
    monkeypatch.setattr(model, '_loss_D', lambda pred, fut: last['d_losses'])
    monkeypatch.setattr(model, '_loss_G', lambda pred, fut: (last['recon'], last['adv']))
    feed = {'image': torch.rand(b, r, r, 3) * 2 - 1, 'future_image': torch.rand(b, r, r, 3) * 2 - 1}
    for idx in (0, 1):
        assert model.test_step(None, feed, 40, idx, b)[:2] == (1.5, 3.5)
    model.close_loggers()
    imgs = ['future_im', 'im', 'current_points', 'future_points', 'future_im_crude', 'future_im_pred', 'mask']
    assert event_sets(event_file(str(tmp_path / 'detector_translator' / 'test'))) == [
        (40, ['D_real', 'D_fake']), (40, ['reconstruction_metric', 'G_adv_loss']), (40, ['%s/image/0' % n for n in imgs])]


def test_motion_generator_event_sets(tmp_path, cpu_image_ops, monkeypatch):
    from kpx_amd.motion_generator_model import MotionGeneratorModel
    b, k = 3, 4
    model = MotionGeneratorModel(_cfg(tmp_path, k), device='cpu')
    model.initialize_loggers(str(tmp_path))
    rs = np.random.RandomState(5)
    pred = torch.from_numpy(rs.uniform(-1, 1, size=(b, 32, 2 * k)).astype(np.float32))
    vals = dict(loss_D_real=0.5, loss_D_fake=0.25, loss_G_recon=8.0, loss_G_kl=0.125, loss_G_adv=2.0)
    feed = {'keypoints': torch.rand(b, k, 2), 'real_seq': torch.rand(b, 32, k, 2), 'action_code': torch.eye(3)[:b]}
    summ = model._summaries(vals, pred, feed)
    model._write_summaries(model.train_writer, 9, summ + [[__import__('kpx_amd').summary.scalar_value('lr', 1e-4)]])
    feed_im = dict(feed, image=torch.rand(b, 128, 128, 3) * 2 - 1)
    model._write_summaries(model.test_writer, 10, model._summaries(vals, pred, feed_im))
    model.close_loggers()
    seqs = ['first_pt', 'predicted_pose_sequence', 'real_pose_sequence']
    train = event_sets(event_file(str(tmp_path / 'motion_generator' / 'train')))
    assert train == [(9, ['D_real', 'D_fake']), (9, ['recon_loss', 'kl_loss', 'G_adv_loss']),
                     (9, ['%s/image/%d' % (n, i) for n in seqs for i in range(2)]), (9, ['lr'])]
    test = event_sets(event_file(str(tmp_path / 'motion_generator' / 'test')))
    assert test[2] == (10, ['%s/image/%d' % (n, i) for n in ['im'] + seqs for i in range(2)])
    img = {v.tag: v.image for v in events_py(event_file(str(tmp_path / 'motion_generator' / 'train')))[3].summary.value}
    assert (img['predicted_pose_sequence/image/0'].height, img['predicted_pose_sequence/image/0'].width) == (64, 2048)
    assert (img['first_pt/image/1'].height, img['first_pt/image/1'].width) == (128, 128)


def test_only_training_models_on_rank_0_open_writers(tmp_path):
    from kpx_amd.detector_translator_model import DetectorTranslatorModel
    model = DetectorTranslatorModel(_cfg(tmp_path), device='cpu', is_training=False)
    model.initialize_loggers(str(tmp_path))
    assert model.train_writer is None and model.test_writer is None
    assert not os.path.exists(str(tmp_path / 'detector_translator' / 'train'))


def test_summary_interval_is_optional():
    import train
    assert train._should_write_summary({'summary_interval': 5}, 10, 0)
    assert not train._should_write_summary({'summary_interval': 5}, 11, 0)
    assert not train._should_write_summary({'summary_interval': 5}, 10, 1)
    assert not train._should_write_summary({}, 0, 0)


# ------------------------------------------------------------------------------------------------ tests: ABI 7 argument checks
def test_abi7_entries_reject_bad_arguments_without_a_gpu():
    from kpx_amd._lib import lib
    a = 1 << 20
    f = lib.kpx_summary_image_u8_f32
    assert f(None, 1, 8, 8, 3, 0, a, a, None) == -1
    assert f(a, 1, 8, 8, 3, 0, None, a, None) == -1
    assert f(a, 1, 8, 8, 3, 0, a, None, None) == -1
    assert f(a, 0, 8, 8, 3, 0, a, a, None) == -1                 # N
    assert f(a, 1, 0, 8, 3, 0, a, a, None) == -1                 # H
    assert f(a, 1, 8, 8, 2, 0, a, a, None) == -1                 # C = 2
    assert f(a, 1, 8, 8, 5, 0, a, a, None) == -1                 # C = 5
    assert f(a, 1, 8, 8, 3, 4, a, a, None) == -1                 # premap
    assert f(a, 1, 8, 8, 3, -1, a, a, None) == -1
    s = lib.kpx_point_seq_strip_rgb_f32
    assert s(None, 2, 32, 5, 64, 64, 14.3, a, 1, a, None) == -1
    assert s(a, 2, 32, 2, 64, 64, 14.3, a, 1, a, None) == -1     # the recolour reads three palette colours
    assert s(a, 2, 32, 65, 64, 64, 14.3, a, 0, a, None) == -1    # K > 64
    assert s(a, 2, 0, 5, 64, 64, 14.3, a, 1, a, None) == -1      # T
    assert s(a, 2, 1025, 5, 64, 64, 14.3, a, 1, a, None) == -1   # T * W > 65536
    assert s(a, 2, 32, 5, 64, 64, 0.0, a, 1, a, None) == -1      # inv_std


def test_ops_argument_checks():
    from kpx_amd import ops
    from kpx_amd._lib import KpxError
    with pytest.raises(KpxError):
        ops.summary_image_u8(torch.zeros(1, 4, 4, 3), 'unit255')                  # CPU tensor: no fallback
    with pytest.raises(KpxError):
        ops.point_seq_strip_rgb(torch.zeros(1, 2, 5, 2), 8, 8, torch.zeros(5, 3))
