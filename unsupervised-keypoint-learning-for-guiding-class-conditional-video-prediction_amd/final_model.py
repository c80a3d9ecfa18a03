"""Full evaluation pipeline (reference: models/final_model.py) -- SURVEY 8f row 1 / BASELINE configs[4]:
detector -> stage-2 vae_decoder (z ~ N(0,1), 32 LSTM steps) -> translator on B*32 frames, inference-mode batch norm.

Outputs are the tensors evaluate.py saves.  With ``point_maps=True`` they include the colourised key-point maps ``current_points``
[B,R,R,3] and ``future_points`` [B,32,R,R,3] (reference :101-110, R = ``image_size``), rendered by one fused kernel per output
(``model_utils.render_point_maps``).  The palette ``self.colors`` is the reference's ``get_n_colors`` (:37) drawn from
``random.Random(colors_seed)``: the reference draws it from the unseeded module-level ``random``, so ``colors_seed=s`` reproduces its
palette after ``random.seed(s)``.  ``z`` can be injected for deterministic parity tests (the reference draws it unseeded, :71).

``run(..., drive=...)`` is the driven rollout (not in the reference): the 32 key-point frames come from outside --
``ops.points_retarget`` on the detected key points and a driver's -- in the place of ``vae_decoder``, and everything after them is the same
code.  It isolates the translator: no z is drawn or read and the stage-2 variables are not touched.

``run(..., frames=32 S, rate=F, resample=...)`` is the long and the smooth rollout (not in the reference).  The motion
generator is fed once and then free-runs for 32 steps, so S calls are chained: segment s >= 1 is ``vae_decoder`` on its own z with the pose
of frame 32 s in the place of the detected one -- in distribution by construction, which free-running the LSTM past step 32 is not.  The 32 S
key-point frames then go through ``ops.points_resample`` (F - 1 frames between every two) and everything downstream runs on T' = 32 S F
frames.  ``frames=32, rate=1`` is the reference's rollout, on the code path it always had.

``FinalModel(posterior=True)`` also declares the stage-2 ``vae_encoder`` (the reference drops it at inference), and ``encode`` reads the
approximate posterior of a real motion from it: logit = [mu | sigma], the input of ``ops.latent_sample`` / ``ops.latent_stats_add``
(DESIGN.md section 2).  ``run(z=ops.latent_sample(logit, None, 0))`` is then the reconstruction.  Without the argument the variable set,
the graphs and every output are what they were.
"""
import logging
import os
import random

import torch

from . import model_utils, networks, ops, variables
from .resample import check_rollout_args
from .base_model import BaseModel
from .variables import Sym

N_FUTURE_FRAMES = 32          # reference :11
IMAGE_SIZE = 128              # reference :12
# The rollout is ~1 500 small launches per call (32 LSTM steps, eight translator slabs): from the second call on a batch shape it is replayed
# as ONE captured HIP graph (KPX_GRAPH=0: enqueue every launch from Python).  The returned tensors then live in the graph's buffers and are
# overwritten by the next run() of the same shape -- evaluate.py consumes them before it calls run() again.
GRAPH = os.environ.get('KPX_GRAPH', '1') != '0'
log = logging.getLogger('kpx')


class FinalModel(BaseModel):
    name = 'final'            # reference :21

    def __init__(self, config, device='cuda', image_size=IMAGE_SIZE, frames_per_launch=256, seed=1234, point_maps=False, colors_seed=0,
                 posterior=False):
        super(FinalModel, self).__init__(False)
        self.posterior = bool(posterior)                # also declare vae_encoder: encode()
        model_config = config['model']
        self.log_dir = config['paths']['log_dir']
        self.n_points = model_config['n_pts']
        self.cell_info = list(model_config['cell_info'])
        self.vae_dim = model_config['vae_dim']
        self.n_action = model_config.get('n_action', 9)
        self.image_size = image_size
        self.heat_size = image_size // 4
        self.frames_per_launch = frames_per_launch      # translator slab size (B*32 frames are processed in slabs)
        self.device = ops.normalize_device(device)
        self.store = variables.VariableStore(device=self.device, seed=seed)
        self._graphs, self._eager_runs, self._graph_failed = {}, {}, False
        self.colors = model_utils.get_n_colors(self.n_points, pastel_factor=0.0, rng=random.Random(colors_seed))   # :37 (factor ignored there too)
        self.point_maps = point_maps
        # fp32 on the device once: TF casts the float64 palette constant to the maps' dtype
        self._colors_dev = torch.tensor(self.colors, dtype=torch.float32, device=self.device) if point_maps else None

    def build(self, inputs=None):
        r, k, b = self.image_size, self.n_points, 2
        with variables.as_default(self.store):
            emb = networks.image_encoder(Sym(b, r, r, 3), False)
            networks.pose_encoder(Sym(b, r, r, 3), k, False, final_res=r)
            networks.vae_decoder(Sym(b, self.vae_dim), Sym(b, 2 * k), Sym(b, self.n_action), self.cell_info, self.vae_dim, k)
            joint = Sym(b, self.heat_size, self.heat_size, (emb[-2].shape[-1] + 2 * k + 3) // 4 * 4)
            networks.translator(joint, False, final_res=r, cin=emb[-2].shape[-1] + 2 * k)
            if self.posterior:            # declared last: the variables above keep their places and their initial values
                networks.vae_encoder(Sym(b, N_FUTURE_FRAMES, 2 * k), Sym(b, 2 * k), Sym(b, self.n_action), self.cell_info, self.vae_dim)
        self.store.materialise()

    def _check_restore(self, arrays, checkpoint_path):
        """posterior=True: a stage-2 checkpoint (one that holds vae_decoder variables) must hold every vae_encoder variable too"""
        if not self.posterior or not any(n.startswith('vae_decoder/') for n in arrays):
            return
        missing = [n for n in self.store.specs if n.startswith('vae_encoder/') and n not in arrays]
        if missing:
            raise ops._lib.KpxError('FinalModel(posterior=True): %s holds the motion generator without its encoder: %s is missing (and %d more); '
                                    'encode() needs a checkpoint of train.py --mode motion_generator with vae_encoder/*'
                                    % (checkpoint_path, missing[0], len(missing) - 1))

    def encode(self, keypoints, real_seq, action_code):
        """The approximate posterior of a real motion: keypoints [B,K,2] (the first pose), real_seq [B,32,K,2], action_code [B,A], the
        training graph's inputs in its layout (MotionGeneratorModel._generate) -> logit fp32 [B, 2 vae_dim] = [mu | sigma], the output of
        ``networks.vae_encoder``.  No gradients, no random numbers.  From the second call on a shape it is one replayed HIP graph, like run():
        the result then lives in the graph's buffer until the next encode() of that shape."""
        if not self.posterior:
            raise ops._lib.KpxError('FinalModel.encode: this model was built without the encoder; construct it with FinalModel(..., posterior=True)')
        b, k, t = (keypoints.shape[0] if isinstance(keypoints, torch.Tensor) and keypoints.dim() else 0), self.n_points, N_FUTURE_FRAMES
        feeds = {'keypoints': (keypoints, (b, k, 2)), 'real_seq': (real_seq, (b, t, k, 2)), 'action_code': (action_code, (b, self.n_action))}
        for name, (v, shape) in feeds.items():
            if b < 1 or not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != shape or v.device != keypoints.device:
                raise ops._lib.KpxError('FinalModel.encode: %s must be an fp32 tensor %s on one device (got %s)'
                                        % (name, [('B' if b < 1 and i == 0 else s) for i, s in enumerate(shape)],
                                           '%s %s on %s' % (tuple(v.shape), v.dtype, v.device) if isinstance(v, torch.Tensor) else type(v).__name__))
        feeds = {name: v for name, (v, _) in feeds.items()}
        if not (GRAPH and not self._graph_failed and keypoints.is_cuda):
            return self._encode_eager(**feeds)
        key = ('encode', b, keypoints.device.index)
        ent = self._graphs.get(key)
        if ent is not None and ent[3] != self.store.version:         # the parameters changed since the capture: as in run()
            del self._graphs[key]
            self._eager_runs[key] = 0
            ent = None
        if ent is None:
            if self._eager_runs.get(key, 0) < 1:                     # one eager run first, as in run()
                self._eager_runs[key] = 1
                return self._encode_eager(**feeds)
            static = {k_: torch.empty_like(v, memory_format=torch.contiguous_format) for k_, v in feeds.items()}
            for k_, v in feeds.items():
                static[k_].copy_(v)
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph):
                    out = self._encode_eager(**static)
            except Exception as e:          # noqa: BLE001 -- whatever the runtime refuses: stay on the eager path
                log.warning('HIP graph capture of the encoder failed (%s: %s); continuing with eager launches', type(e).__name__, e)
                self._graph_failed = True
                torch.cuda.synchronize(keypoints.device)
                self.store.touch()
                ops.reset_after_failed_capture()
                return self._encode_eager(**feeds)
            ent = self._graphs[key] = (graph, static, out, self.store.version)
        graph, static, out, _ = ent
        for k_, v in feeds.items():
            v = v.contiguous()
            ops.flat_copy_raw(v.data_ptr(), static[k_].data_ptr(), v.numel())
        graph.replay()
        return out

    def _encode_eager(self, keypoints, real_seq, action_code):
        """encode() enqueued launch by launch (also the function a capture records)"""
        b, k2 = keypoints.shape[0], 2 * self.n_points
        with variables.as_default(self.store), torch.no_grad():
            return networks.vae_encoder(real_seq.reshape(b, N_FUTURE_FRAMES, k2), keypoints.reshape(b, k2).contiguous(), action_code.contiguous(),
                                        self.cell_info, self.vae_dim)

    def run(self, sess, feed_dict, z=None, drive=None, frames=N_FUTURE_FRAMES, rate=1, resample='cubic'):
        """reference run (:124-125).  feed_dict: {'image': [B,H,W,3] in [-1,1], 'action_code': [B,n_action] one-hot,
        optional 'real_im_seq', 'real_seq'}.  z: the VAE latent [B, vae_dim]; drawn from N(0,1) when not given (:71).
        drive: {'mode': 'hold' | 'absolute' | 'relative', 'first': [B,K,2], 'seq': [B,32,K,2], 'shift': int, 'scaled': bool} -- the 32
        key-point frames come from ``ops.points_retarget`` on the detected key points instead of the motion generator ('first' and 'seq'
        are the driver's key points at frame 0 and at frames 1..32, absent for 'hold'; 'first' is read by 'relative' alone; sample b is
        driven by sample (b + shift) mod B).  z and 'action_code' are then neither drawn nor read.
        frames: a positive multiple of 32; S = frames / 32 chained motion-generator segments, z then [S,B,vae_dim] ([B,vae_dim] serves S = 1),
        drawn once as [S,B,vae_dim] when not given.  rate: F in [1, 64]; the frames * F key-point frames are ``ops.points_resample`` of the
        frames knots in the mode ``resample`` ('linear' | 'cubic').  Every [B,32,...] output then has T' = frames * F frames.  A driven
        rollout takes rate (the 32 retargeted frames are resampled) and refuses frames != 32: a driver has 33 frames."""
        segments, _ = check_rollout_args('FinalModel.run', frames, rate, resample)
        if drive is not None:
            if segments != 1:
                raise ops._lib.KpxError('FinalModel.run: frames must be %d with drive= (got %r): a driver has %d frames and nothing chains it'
                                        % (N_FUTURE_FRAMES, frames, N_FUTURE_FRAMES + 1))
            return self._run_driven(feed_dict, drive, rate, resample)
        if segments != 1 or rate != 1:
            return self._run_long(feed_dict, z, segments, rate, resample)
        im, act = feed_dict['image'], feed_dict['action_code']
        if not (GRAPH and not self._graph_failed and im.is_cuda and im.dtype == torch.float32):
            return self._run_eager(feed_dict, z)
        if z is None:
            z = torch.randn((im.shape[0], self.vae_dim), dtype=torch.float32, device=im.device)              # :71 (drawn outside the graph)
        key = (tuple(im.shape), tuple(act.shape), im.device.index)
        ent = self._graphs.get(key)
        if ent is not None and ent[3] != self.store.version:
            # The parameters changed since the capture (restore / load_numpy / assign -> VariableStore.touch()).  The graph holds the
            # ADDRESSES of the batch-norm-folded filters and their Winograd forms, which touch() released: replaying it would read freed
            # memory.  Drop it; the eager run below re-derives them for the new parameters and the next call captures again.
            del self._graphs[key]
            self._eager_runs[key] = 0
            ent = None
        if ent is None:
            if self._eager_runs.get(key, 0) < 1:                     # one eager run first: it creates every lazily allocated buffer / attribute
                self._eager_runs[key] = 1
                return self._run_eager(feed_dict, z)
            static = {'image': torch.empty_like(im, memory_format=torch.contiguous_format), 'action_code': torch.empty_like(act, memory_format=torch.contiguous_format),
                      'z': torch.empty_like(z, memory_format=torch.contiguous_format)}
            for k_, v in (('image', im), ('action_code', act), ('z', z)):
                static[k_].copy_(v)
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph):
                    out = self._run_eager({'image': static['image'], 'action_code': static['action_code']}, static['z'])
            except Exception as e:          # noqa: BLE001 -- whatever the runtime refuses: stay on the eager path
                log.warning('HIP graph capture of the rollout failed (%s: %s); continuing with eager launches', type(e).__name__, e)
                self._graph_failed = True
                torch.cuda.synchronize(im.device)
                self.store.touch()          # host bookkeeping advanced for launches that were only recorded: derive everything again
                ops.reset_after_failed_capture()
                return self._run_eager(feed_dict, z)
            ent = self._graphs[key] = (graph, static, out, self.store.version)
        graph, static, out, _ = ent
        for k_, v in (('image', im), ('action_code', act), ('z', z)):
            v = v.contiguous()
            ops.flat_copy_raw(v.data_ptr(), static[k_].data_ptr(), v.numel())
        graph.replay()
        res = dict(out)
        res['im'] = im
        res['real_im_seq'] = feed_dict.get('real_im_seq')
        return res

    def detect(self, image):
        """The detector alone (animate.py --driver): image [B,R,R,3] in [-1,1] -> its key points [B,K,2] as (x, y), the ``first_pt`` of run()."""
        im = image.contiguous()
        with variables.as_default(self.store), torch.no_grad():
            return networks.pose_encoder(im, self.n_points, False, final_res=self.image_size).reshape(im.shape[0], self.n_points, 2)

    def _check_drive(self, im, drive):
        """-> (mode, shift, scaled, {'first' / 'seq': contiguous tensors the mode reads}); everything ops.points_retarget would refuse is
        refused here, before any copy into a graph's static buffers"""
        if not isinstance(drive, dict) or set(drive) - {'mode', 'first', 'seq', 'shift', 'scaled'}:
            raise ops._lib.KpxError("FinalModel.run: drive is a dict of 'mode', 'first', 'seq', 'shift' and 'scaled' (got %r)"
                                    % (sorted(drive) if isinstance(drive, dict) else type(drive).__name__,))
        mode, shift, scaled = drive.get('mode'), drive.get('shift', 0), drive.get('scaled', False)
        b, k, t = im.shape[0], self.n_points, N_FUTURE_FRAMES
        if mode not in ops.RETARGET_MODES:
            raise ops._lib.KpxError('FinalModel.run: drive mode must be one of %s (got %r)' % (sorted(ops.RETARGET_MODES), mode))
        if isinstance(shift, bool) or not isinstance(shift, int) or not 0 <= shift < b:
            raise ops._lib.KpxError('FinalModel.run: drive shift must be an integer in [0, B = %d) (got %r)' % (b, shift))
        if not isinstance(scaled, bool) or (scaled and mode != 'relative'):
            raise ops._lib.KpxError("FinalModel.run: drive scaled is a bool and belongs to mode 'relative' (got %r for %r)" % (scaled, mode))
        if mode == 'hold' and ('first' in drive or 'seq' in drive):
            raise ops._lib.KpxError("FinalModel.run: drive mode 'hold' takes no 'first' or 'seq'")
        tensors = {}
        for name, shape in (('first', (b, k, 2)), ('seq', (b, t, k, 2))):
            if mode == 'hold' or (name == 'first' and mode != 'relative'):
                continue
            v = drive.get(name)
            if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.device != im.device or tuple(v.shape) != shape:
                raise ops._lib.KpxError('FinalModel.run: drive %r must be an fp32 tensor %s on %s (got %s)'
                                        % (name, list(shape), im.device, '%s %s on %s' % (tuple(v.shape), v.dtype, v.device)
                                           if isinstance(v, torch.Tensor) else type(v).__name__))
            tensors[name] = v.contiguous()
        return mode, shift, scaled, tensors

    def _run_driven(self, feed_dict, drive, rate=1, resample='cubic'):
        """run(drive=...): as run(), with the driver's key points in the place of z.  The scalars (mode, shift, scaled) are launch arguments
        of the captured points_retarget, so they are part of the graph's key."""
        im, act = feed_dict['image'], feed_dict.get('action_code')
        mode, shift, scaled, tensors = self._check_drive(im, drive)
        eager = lambda image, ts: self._run_eager({'image': image}, drive=dict(ts, mode=mode, shift=shift, scaled=scaled), rate=rate, resample=resample)
        if not (GRAPH and not self._graph_failed and im.is_cuda and im.dtype == torch.float32):
            return dict(eager(im, tensors), real_im_seq=feed_dict.get('real_im_seq'))
        key = (tuple(im.shape), None if act is None else tuple(act.shape), im.device.index, mode, shift, scaled)
        if rate != 1:                 # the rate and the mode are launch arguments of the captured points_resample
            key += (rate, resample)
        feeds = dict(tensors, image=im)
        ent = self._graphs.get(key)
        if ent is not None and ent[3] != self.store.version:         # the parameters changed since the capture: as in run()
            del self._graphs[key]
            self._eager_runs[key] = 0
            ent = None
        if ent is None:
            if self._eager_runs.get(key, 0) < 1:                     # one eager run first, as in run()
                self._eager_runs[key] = 1
                return dict(eager(im, tensors), real_im_seq=feed_dict.get('real_im_seq'))
            static = {k_: torch.empty_like(v, memory_format=torch.contiguous_format) for k_, v in feeds.items()}
            for k_, v in feeds.items():
                static[k_].copy_(v)
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph):
                    out = eager(static['image'], {k_: static[k_] for k_ in tensors})
            except Exception as e:          # noqa: BLE001 -- whatever the runtime refuses: stay on the eager path
                log.warning('HIP graph capture of the driven rollout failed (%s: %s); continuing with eager launches', type(e).__name__, e)
                self._graph_failed = True
                torch.cuda.synchronize(im.device)
                self.store.touch()
                ops.reset_after_failed_capture()
                return dict(eager(im, tensors), real_im_seq=feed_dict.get('real_im_seq'))
            ent = self._graphs[key] = (graph, static, out, self.store.version)
        graph, static, out, _ = ent
        for k_, v in feeds.items():
            v = v.contiguous()
            ops.flat_copy_raw(v.data_ptr(), static[k_].data_ptr(), v.numel())
        graph.replay()
        res = dict(out)
        res['im'] = im
        res['real_im_seq'] = feed_dict.get('real_im_seq')
        return res

    def _run_long(self, feed_dict, z, segments, rate, resample):
        """run(frames=32 * segments, rate=, resample=) without a driver: as run(), with z [S,B,V] and (frames, rate, resample) in the graph's key
        (they decide the launches a capture records)."""
        im, act = feed_dict['image'], feed_dict['action_code']
        b = im.shape[0]
        if z is None:
            z = torch.randn((segments, b, self.vae_dim), dtype=torch.float32, device=im.device)           # drawn once, outside the graph
        elif isinstance(z, torch.Tensor) and z.dim() == 2 and segments == 1:
            z = z.reshape(1, b, self.vae_dim)
        if not isinstance(z, torch.Tensor) or z.dtype != torch.float32 or z.device != im.device or tuple(z.shape) != (segments, b, self.vae_dim):
            raise ops._lib.KpxError('FinalModel.run: z must be an fp32 tensor %s on %s for frames = %d (got %s)'
                                    % ([segments, b, self.vae_dim], im.device, N_FUTURE_FRAMES * segments,
                                       '%s %s on %s' % (tuple(z.shape), z.dtype, z.device) if isinstance(z, torch.Tensor) else type(z).__name__))
        frames = N_FUTURE_FRAMES * segments
        eager = lambda image, action, z_: self._run_eager({'image': image, 'action_code': action}, z_, frames=frames, rate=rate, resample=resample)
        if not (GRAPH and not self._graph_failed and im.is_cuda and im.dtype == torch.float32):
            return dict(eager(im, act, z), real_im_seq=feed_dict.get('real_im_seq'))
        key = (tuple(im.shape), tuple(act.shape), im.device.index, 'long', frames, rate, resample)
        feeds = {'image': im, 'action_code': act, 'z': z}
        ent = self._graphs.get(key)
        if ent is not None and ent[3] != self.store.version:         # the parameters changed since the capture: as in run()
            del self._graphs[key]
            self._eager_runs[key] = 0
            ent = None
        if ent is None:
            if self._eager_runs.get(key, 0) < 1:                     # one eager run first, as in run()
                self._eager_runs[key] = 1
                return dict(eager(im, act, z), real_im_seq=feed_dict.get('real_im_seq'))
            static = {k_: torch.empty_like(v, memory_format=torch.contiguous_format) for k_, v in feeds.items()}
            for k_, v in feeds.items():
                static[k_].copy_(v)
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph):
                    out = eager(static['image'], static['action_code'], static['z'])
            except Exception as e:          # noqa: BLE001 -- whatever the runtime refuses: stay on the eager path
                log.warning('HIP graph capture of the long rollout failed (%s: %s); continuing with eager launches', type(e).__name__, e)
                self._graph_failed = True
                torch.cuda.synchronize(im.device)
                self.store.touch()
                ops.reset_after_failed_capture()
                return dict(eager(im, act, z), real_im_seq=feed_dict.get('real_im_seq'))
            ent = self._graphs[key] = (graph, static, out, self.store.version)
        graph, static, out, _ = ent
        for k_, v in feeds.items():
            v = v.contiguous()
            ops.flat_copy_raw(v.data_ptr(), static[k_].data_ptr(), v.numel())
        graph.replay()
        res = dict(out)
        res['im'] = im
        res['real_im_seq'] = feed_dict.get('real_im_seq')
        return res

    def _chained_points(self, z, first_pt, act, segments):
        """The key points of a chained rollout, fp32 [B, 32 S, 2K]: segment 0 is vae_decoder on the detected pose, segment s >= 1 on the pose of
        frame 32 s, each with its own z[s] and the same action code.  Copies only between the calls (kpx_copy_channels)."""
        b, k2, t = first_pt.shape[0], 2 * self.n_points, N_FUTURE_FRAMES
        knots = torch.empty((b, segments * t, k2), dtype=torch.float32, device=first_pt.device)
        f_pt = first_pt.reshape(b, k2)
        for s in range(segments):
            seg = networks.vae_decoder(z[s], f_pt, act, self.cell_info, self.vae_dim, self.n_points)          # [B,32,2K]
            ops.copy_channels_raw(seg.data_ptr(), t * k2, knots.data_ptr() + 4 * s * t * k2, segments * t * k2, b, t * k2)
            if s + 1 < segments:
                f_pt = torch.empty((b, k2), dtype=torch.float32, device=first_pt.device)
                ops.copy_channels_raw(seg.data_ptr() + 4 * (t - 1) * k2, t * k2, f_pt.data_ptr(), k2, b, k2)
        return knots

    def _run_eager(self, feed_dict, z=None, drive=None, frames=N_FUTURE_FRAMES, rate=1, resample='cubic'):
        """The rollout enqueued launch by launch (also the function a capture records).  ``drive``: a checked drive dict (_check_drive).
        ``frames``, ``rate``, ``resample``: checked by run(); z is [S,B,V] when frames > 32."""
        im = feed_dict['image'].contiguous()
        act = feed_dict['action_code'].contiguous() if drive is None else None
        b, r, k, t = im.shape[0], self.image_size, self.n_points, N_FUTURE_FRAMES
        segments = frames // t
        dev = im.device
        with variables.as_default(self.store), torch.no_grad():
            emb = networks.image_encoder(im, False)[-2]                                          # :61-62
            first_pt = networks.pose_encoder(im, k, False, final_res=r)                          # :68
            if drive is not None:             # the driven rollout: the key points come from outside, no z
                pred_seq = ops.points_retarget(first_pt.reshape(b, k, 2).contiguous(), drive['mode'], drive.get('first'), drive.get('seq'),
                                               shift=drive['shift'], scaled=drive['scaled'], frames=t if drive['mode'] == 'hold' else None)
            else:
                if z is None:
                    z = torch.randn((b, self.vae_dim), dtype=torch.float32, device=dev)          # :71
                if segments == 1:
                    pred_seq = networks.vae_decoder(z if z.dim() == 2 else z[0], first_pt.reshape(b, 2 * k), act, self.cell_info, self.vae_dim, k)   # :72-77
                else:
                    if z.dim() == 2:
                        raise ops._lib.KpxError('FinalModel: a rollout of %d frames takes z [%d, B, vae_dim]' % (frames, segments))
                    pred_seq = self._chained_points(z, first_pt, act, segments)
            if rate != 1:                     # F - 1 frames between every two knots; the knots themselves stay, bit for bit
                pred_seq = ops.points_resample(first_pt.reshape(b, k, 2).contiguous(), pred_seq.reshape(b, frames, k, 2), rate, resample)
            t = frames * rate                 # T': everything downstream runs on it
            pred_pts = pred_seq.reshape(b * t, k, 2)
            # joint embedding [B*T, h, h, C+2K (+pad)]: tiled image embedding ‖ tiled current map ‖ per-frame predicted map
            c = emb.shape[-1]
            ld = (c + 2 * k + 3) // 4 * 4
            hs = self.heat_size
            finals, crudes, masks = [], [], []
            first_tiled = ops.tile_batch(first_pt.reshape(b, 1, 2 * k), t).reshape(b * t, k, 2)   # :85-87 (points instead of maps)
            if t <= max(self.frames_per_launch, N_FUTURE_FRAMES):
                fpl = max(t, (self.frames_per_launch // t) * t)      # whole samples per slab
                slabs = [(s, min(b * t, s + fpl), t) for s in range(0, b * t, fpl)]
            else:                             # a long rollout: a sample's frames no longer fit one slab, so a slab is a run of one sample's frames
                slabs = [(i * t + s, i * t + min(t, s + self.frames_per_launch), min(t, s + self.frames_per_launch) - s)
                         for i in range(b) for s in range(0, t, self.frames_per_launch)]
            for s, e, rep_ in slabs:          # rows s..e of the B*T' frames: (e - s) / rep_ samples, rep_ frames of each
                nb = (e - s) // rep_
                joint = torch.empty((e - s, hs, hs, ld), dtype=torch.float32, device=dev)
                if ld > c + 2 * k:
                    ops.fill_raw_(joint, 0.0)
                ops.tile_batch(emb[s // t:s // t + nb], rep_, out=joint, out_ld=ld, out_channel_offset=0)          # :63-66
                for i, pts in enumerate((first_tiled[s:e], pred_pts[s:e])):                                        # :79-92
                    ops.check(ops.lib.kpx_gaussian_maps_fwd_f32(pts.contiguous().data_ptr(), e - s, k, hs, hs, 14.3,
                                                                joint.data_ptr() + 4 * (c + i * k), ld, ops._stream()),
                              'kpx_gaussian_maps_fwd_f32')
                raw4 = networks.translator(joint, False, final_res=r, cin=c + 2 * k)                                # :95
                f_, c_, m_ = ops.head_blend_tiled(im[s // t:s // t + nb], raw4, rep_, clip=True)                    # :96-99
                finals.append(f_); crudes.append(c_); masks.append(m_)
            cat = lambda xs: xs[0] if len(xs) == 1 else torch.cat(xs, dim=0)
            out = {'im': im, 'real_im_seq': feed_dict.get('real_im_seq'),
                   'pred_im_seq': cat(finals).reshape(b, t, r, r, 3), 'mask': cat(masks).reshape(b, t, r, r, 1),
                   'pred_im_crude': cat(crudes).reshape(b, t, r, r, 3), 'fut_pt_raw': pred_seq.reshape(b, t, k, 2),
                   'first_pt': first_pt}
            if self.point_maps:                                                                  # :101-110
                out['current_points'] = model_utils.render_point_maps(first_pt.reshape(b, k, 2), (r, r), self._colors_dev)
                out['future_points'] = model_utils.render_point_maps(pred_pts, (r, r), self._colors_dev).reshape(b, t, r, r, 3)
            return out

    def train_step(self, sess, feed_dict, step, batch_size, should_write_log=False, should_write_summary=False):
        raise NotImplementedError          # reference :127-136

    def test_step(self, sess, feed_dict, step, test_idx, batch_size):
        raise NotImplementedError

    def collect_test_results(self, results, step):
        raise NotImplementedError
