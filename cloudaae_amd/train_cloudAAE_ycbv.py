"""Training step -- mirror of the reference's train_cloudAAE_ycbv.py (setup_graph :137-329,
train_graph :332-437, CLI :440-484), MI355X-native.

What the reference assembles as a TF graph (:194-273) is `TrainGraph.forward` here; one
`TrainGraph.train_step(batch)` is one iteration of the reference's session loop (:350-368):
bn_decay schedule -> input assembly -> model -> three losses -> gradients -> Adam.
Everything between the input batch and the updated weights runs in libcloudaae_hip.so on
the GPU; step counter, Adam beta powers and the BN decay are device scalars, so a step
issues no host synchronisation.

Data parallelism (new; the reference is single-GPU): one process per GPU, the batch is
sharded across ranks, gradients are averaged with RCCL all-reduce over the store's flat
gradient buffer -- the 12.6 M-element dgcnn_output weight gradient, produced first in
backward, is reduced asynchronously while the encoder backward still runs.  Batch-norm
statistics are per-rank (local BN).
"""
import argparse
import importlib
import math
import os
import re
import time

import torch
import torch.distributed as dist

from . import _lib
from ._lib import ptr, require, stream
from .losses import angular_distance_taylor, chamfer_loss, trans_distance
from .utils import _functions as F
from .utils import tf_util
from .utils.grad_exchange import GradExchange
from .utils.variables import reset_default_store, set_default_store

NUM_CLASS = 21                      # train_cloudAAE_ycbv.py:29
BN_INIT_DECAY = 0.5                 # :166-169
BN_DECAY_DECAY_RATE = 0.5
BN_DECAY_DECAY_STEP = float(40)
BN_DECAY_CLIP = 0.99
NOISE_STDDEV = 0.004 / 3.           # :217
LOSS_WEIGHTS = (1000.0, 10.0, 1.0)  # :268
K_NEIGHBOR = 10                     # :230
EMA_NAME_SCOPE = 'decoder'          # tf.name_scope the model is built under (:223)


def get_training_argparser():
    """Same flags as train_cloudAAE_ycbv.py:440-467, plus the data-parallel/benchmark ones."""
    parser = argparse.ArgumentParser()
    general = parser.add_argument_group('general')
    general.add_argument('--gpu', type=int, default=0, help='GPU to use [default: GPU 0]')
    general.add_argument('--model', default='pointnet_ycb_23_decoder_4', help='Model module name')
    general.add_argument('--log_dir', default='log', help='Log dir [default: log]')
    general.add_argument('--num_point', type=int, default=256, help='Point Number [256/512/1024] [default: 256]')
    general.add_argument('--total_num_point', type=int, default=512, help='Dataset Point Number')
    train_opts = parser.add_argument_group('training_options')
    train_opts.add_argument('--max_epoch', type=int, default=500, help='Epoch to run')
    train_opts.add_argument('--optimizer', default='adam', help='adam or gd [default: adam]')
    hyper = parser.add_argument_group('hyperparameters')
    hyper.add_argument('--batch_size', type=int, default=128, help='Batch Size during training [default: 128]')
    hyper.add_argument('--learning_rate', type=float, default=0.0008, help='Initial learning rate')
    hyper.add_argument('--momentum', type=float, default=0.9)
    hyper.add_argument('--decay_step', type=int, default=30000)
    hyper.add_argument('--decay_rate', type=float, default=0.7)
    hyper.add_argument('--trans_tol', type=float, default=0.1)
    extra = parser.add_argument_group('mi355x')
    extra.add_argument('--model_fn', default='get_model_dgcnn_mean_6d')
    extra.add_argument('--k', type=int, default=K_NEIGHBOR)
    extra.add_argument('--steps', type=int, default=0,
                       help='batches per epoch (0 = the whole epoch); synthetic steps without --data_dir (0 = 100)')
    extra.add_argument('--data_dir', default='', help='directory holding object_model_tfrecord/ and '
                       'ycb_video_data_tfRecords/train_syn/ (:31-39); empty = synthetic batches')
    extra.add_argument('--restore', default='', help='checkpoint to resume from: a TensorFlow V2 prefix (model.ckpt) or an .npz')
    extra.add_argument('--ckpt_format', default='npz', choices=['npz', 'tf'], help="format of the epoch checkpoints")
    extra.add_argument('--gemm_dtype', default='bf16x3', help="bf16x3 (default) = fp32 everywhere, the three dgcnn_agg products computed as error-free "
                            "3 x bfloat16 split products on the bf16 matrix cores (fp32 accuracy); f32 = those products on the fp32 "
                            "matrix cores too; bf16 = bf16 operands for the dense layers (BASELINE configs[2])")
    extra.add_argument('--print_every', type=int, default=1, help='print the losses every n batches (each print syncs)')
    extra.add_argument('--poses', default='records', choices=['records', 'sampled'],
                       help="records: the pose records of --data_dir (train_syn); sampled: poses drawn on the GPU "
                            "(utils/sample_pose_in_frustum.py), which needs object models only")
    extra.add_argument('--occluder', default='spherical', choices=['spherical', 'object'],
                       help="the two Gaussian blobs, or 512 points of a rotated object model (utils/generate_occluder.py)")
    extra.add_argument('--dataset', default='ycbv', choices=['ycbv', 'linemod'], help='camera and frustum constants')
    extra.add_argument('--epoch_size', type=int, default=381553,
                       help='samples per epoch with --poses sampled [default: the shipped train_syn set]')
    extra.add_argument('--classes', default='', help='comma-separated class ids to train on [default: all]')
    extra.add_argument('--pose_seed', type=int, default=123456789, help='seed of the sampled poses')
    extra.add_argument('--deterministic', action='store_true', help='bit-reproducible steps (TrainGraph(deterministic=True))')
    extra.add_argument('--meshes', default='', help='directory of *.ply meshes to build the object models from on the GPU '
                       '(utils/mesh_models.py; class i is the i-th file in sorted order); with --poses sampled only')
    extra.add_argument('--mesh_scale', type=float, default=1.0,
                       help='factor on the mesh coordinates (0.001 for meshes in millimetres)')
    extra.add_argument('--visibility', default='hpr', choices=['hpr', 'rendered'],
                       help="hpr: hidden point removal on the sampled object models; rendered: clouds drawn from depth "
                            "frames of the --meshes rendered behind a mesh occluder (utils/rendered_data.py); with --poses "
                            "sampled and --meshes only [default: hpr]")
    extra.add_argument('--sensor', default='none', choices=['none', 'kinect1'],
                       help='depth sensor model on the rendered frames (utils/depth_noise.py); with --visibility rendered')
    extra.add_argument('--sensor_seed', type=int, default=0, help='seed of the sensor noise')
    extra.add_argument('--symmetries', default='none',
                       help="none: the pose labels as they are [default]; auto: find the rotational symmetries of the classes "
                            "trained on (of the --meshes, else of the class models) and train against the nearest equivalent "
                            "label (utils/pose_equiv.py); or the JSON file python -m cloudaae_amd.utils.symmetry wrote")
    return parser


def parse_arg_groups(parser, argv=None):
    """train_cloudAAE_ycbv.py:470-475."""
    args = parser.parse_args(argv)
    arg_groups = {}
    for group in parser._action_groups:
        arg_groups[group.title] = {a.dest: getattr(args, a.dest, None) for a in group._group_actions}
    return arg_groups


class TrainGraph(object):
    """The counterpart of setup_graph(): owns the variables, the optimiser slots and the
    device-side bookkeeping scalars; `forward` is the graph of :206-268."""

    def __init__(self, general_opts=None, train_opts=None, hyperparameters=None, device=None,
                 model_fn='get_model_dgcnn_mean_6d', k_neighbor=K_NEIGHBOR, process_group=None, seed=123456789,
                 replay=False, gemm_dtype='bf16x3', side_stream=None, sync_bn=False, deterministic=False,
                 symmetries=None):
        general_opts = dict(general_opts or {})
        train_opts = dict(train_opts or {})
        hyperparameters = dict(hyperparameters or {})
        self.NUM_POINT = int(general_opts.get('num_point', 256))
        self.BATCH_SIZE = int(hyperparameters.get('batch_size', 128))          # GLOBAL batch
        self.BASE_LEARNING_RATE = float(hyperparameters.get('learning_rate', 0.0008))
        self.OPTIMIZER = train_opts.get('optimizer', 'adam')
        require(self.OPTIMIZER in ('adam', 'gd'), "optimizer must be adam or gd")
        self.device = torch.device(device if device is not None else 'cuda:%d' % int(general_opts.get('gpu', 0)))
        self.k = int(k_neighbor)
        # side_stream: weight-gradient products of the per-point layers and the reverse neighbour lists on
        # the library's low-priority stream.  OFF by default: measured SLOWER at B=32 (2.35 ms/step with
        # every edge-conv layer using it, 2.32 with only the dgcnn_agg weight gradient, 2.25 without) --
        # the concurrent GEMM takes L2 and CUs from the gather-bound kernels it overlaps, and every
        # cross-stream dependency costs microseconds.  CLOUDAAE_SIDE_STREAM=1 (or =agg) switches it on.
        self.side_stream = (os.environ.get("CLOUDAAE_SIDE_STREAM", "0") != "0") if side_stream is None \
            else bool(side_stream)
        # process_group: None = the default group when torch.distributed is initialised;
        # False = single-process even then; or an explicit group
        solo = process_group is False or not (dist.is_available() and dist.is_initialized())
        self.pg = None if solo else process_group
        self.world = 1 if solo else dist.get_world_size(self.pg)
        self.rank = 0 if solo else dist.get_rank(self.pg)
        require(self.BATCH_SIZE % self.world == 0, "global batch must divide by the number of ranks")
        self.local_batch = self.BATCH_SIZE // self.world
        # sync_bn: batch-norm moments (and their gradients) over the GLOBAL batch -- what the single-GPU
        # reference computes (utils/tf_util.py:492: tf.nn.moments over the whole batch), so that an N-rank
        # run equals a 1-rank run of the global batch; default: per-rank moments (local BN)
        # (CLOUDAAE_FORCE_COLLECTIVES=1: also with one rank, to exercise the RCCL path on a single-GPU box)
        forced = not solo and os.environ.get("CLOUDAAE_FORCE_COLLECTIVES") == "1"
        self.sync_bn = bool(sync_bn) and (self.world > 1 or forced)
        self.bn_sync = None
        if self.sync_bn:
            from .utils.sync_bn import BnSync
            self.bn_sync = BnSync(self.pg, self.world)
        # MODEL = importlib.import_module(general_opts['model'])   (:147) -- the plugin seam
        self.MODEL = importlib.import_module('cloudaae_amd.models.' +
                                             general_opts.get('model', 'pointnet_ycb_23_decoder_4'))
        self.model_fn = getattr(self.MODEL, model_fn)
        self.is_pn = model_fn == 'get_model_pn'

        torch.cuda.set_device(self.device)
        self.store = reset_default_store(device=self.device, seed=seed)   # tf.set_random_seed(123456789), :160
        dev = self.device
        self.batch = torch.zeros(1, dtype=torch.float32, device=dev)         # `batch = tf.Variable(0.)`, :192
        self.bn_decay = torch.full((1,), 0.5, dtype=torch.float32, device=dev)
        self.beta1_power = torch.full((1,), 0.9, dtype=torch.float32, device=dev)
        self.beta2_power = torch.full((1,), 0.999, dtype=torch.float32, device=dev)
        self._one = torch.ones((), dtype=torch.float32, device=dev)           # d(total_loss)/d(total_loss)
        # seed of this rank's input noise (:217; tf.set_random_seed(123456789), :160)
        self.noise_seed = (int(seed) + 0x9E3779B97F4A7C15 * (self.rank + 1)) % (1 << 64)
        self.noise_draws = torch.zeros(2, dtype=torch.int64, device=dev)     # {draw counter, ticket} of the assembly kernel
        self._adam_ticket = torch.zeros(1, dtype=torch.int32, device=dev)   # arrival counter of the optimiser kernel
        # replay=True: the first train_step of a given input shape is RECORDED (_lib.StepPlan: the
        # C-ABI calls in issue order, buffers from the plan's arena) and later steps re-issue it
        # without Python layers or autograd in between -- the host cost of a step drops from ~3 ms
        # to the launches themselves, which is what keeps a batch-32 step GPU-bound.
        # gemm_dtype='bf16x3' (default): an fp32 step; the three dgcnn_agg products (tf_util.py:161-166 and its two gradient
        # products, 29 % of an fp32-MFMA step) split every operand element EXACTLY into three bfloat16 pieces and take the
        # six piece products of weight >= 2^-16 on the bf16 matrix cores, fp32 accumulate -- what is dropped is below one
        # fp32 rounding of each product (csrc/gemm_x3.hip; tests: test_gemm_bf16x3*, cfg1-B32 at the fp32 tolerances).
        # 'f32': the same products on v_mfma_f32_32x32x2_f32.
        # gemm_dtype='bf16': the per-point conv1x1 products (and their gradient products) round their operands
        # to bfloat16 on the way to the matrix cores, fp32 accumulate; everything else -- tensors in
        # HBM, batch norm, kNN, Chamfer, pose losses, Adam -- stays fp32 (BASELINE configs[2])
        require(gemm_dtype in ('f32', 'bf16', 'bf16x3'), "gemm_dtype must be 'f32', 'bf16' or 'bf16x3'")
        self.gemm_dtype = gemm_dtype
        # deterministic=True: the whole step is bit-reproducible from run to run, as the reference's sequential CPU path
        # is (tf_ops/nn_distance/tf_nndistance.cpp:21-43, 126-163).  The forward pass always is (every forward product is
        # summed in a fixed order); this flag also takes the fp32 atomics out of the backward pass -- products whole over
        # K, the fully connected stack through GEMM + batch norm, the Chamfer gradient in the reference's CPU order, sorted
        # reverse neighbour lists -- at a price (measured: DESIGN.md).  One process, one mode: the library's knob is
        # process-wide and set at every step.
        self.deterministic = bool(deterministic)
        # symmetries: a pose_equiv.SymmetryTable.  The pose terms are then taken against the label that is equivalent
        # under the object's symmetries and nearest the predicted rotation -- the minimum of the loss over the symmetry
        # set, the choice held constant in the gradient -- found by one launch in front of the loss (DESIGN.md,
        # "Equivalent poses").  None: the element's labels as they are, and not one call more.
        self.replay = bool(replay)
        self.reuse_staged_inputs = False
        self._plan = self._plan_key = self._plan_out = self._static = self._staged = None
        self._plans = {}                     # parked recordings of other input shapes
        self.symmetries = None
        if symmetries is not None:
            self.set_symmetries(symmetries)
        self._build()

    def set_symmetries(self, table):
        """Give the graph a symmetry table (or None) after construction, e.g. once the object models are known.  Steps
        recorded so far are dropped: the launch is part of a recorded step."""
        if table is not None:
            from .utils.pose_equiv import SymmetryTable
            require(isinstance(table, SymmetryTable), "symmetries must be a pose_equiv.SymmetryTable or None")
            table.on(self.device)
        self.symmetries = table
        self._plan = self._plan_key = self._plan_out = self._static = self._staged = None
        self._plans = {}

    # -- graph construction: create every variable once, then pack them ---------------------
    def _build(self):
        B, N = max(2, min(self.local_batch, 2)), self.NUM_POINT
        dummy = torch.zeros((B, N, 3 + NUM_CLASS), dtype=torch.float32, device=self.device)
        dummy[:, :, :3] = torch.rand((B, N, 3), device=self.device)
        with torch.no_grad():
            self._call_model(dummy, False)
        # the fully connected stack (tag 'fc': decoder + pose heads) goes to the END of the flat buffers: its
        # gradients are the first ones backward produces, and the exchange reduces them as one early piece
        self.store.flatten(last=lambda v: v.tag == 'fc')
        n = self.store.flat_params.numel()
        self.adam_m = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.adam_v = torch.zeros(n, dtype=torch.float32, device=self.device)
        fc = [v for v in self.store.trainable_variables() if v.tag == 'fc']
        early = None
        if fc:
            lo = min(self.store.offsets[v.name] for v in fc)
            early = (lo, n)
        self.exchange = GradExchange(self.store.flat_grads, early, self.pg, world=self.world, early_count=len(fc))
        # (with SyncBN the fully connected stack runs as product + batch norm, whose split-K products ADD)
        self._set_mode()
        self._zero_limit = early[0] if (early is not None and F.fc_fits(self.local_batch) and not self.sync_bn) else None
        self.exchange.broadcast_params(self.store.flat_params)     # identical initial weights on every rank
        if early is not None and self.exchange.active:
            for v in fc:
                v.on_ready = self.exchange.early_ready

    def _set_mode(self):
        F.DETERMINISTIC = self.deterministic
        _lib.set_knob("CLOUDAAE_DETERMINISTIC", 1 if self.deterministic else None)

    def _call_model(self, pc, is_training):
        set_default_store(self.store)      # several graphs may live in one process (cf. tf.Graph.as_default)
        self._set_mode()
        F.GEMM_DTYPE = self.gemm_dtype     # read by every dense layer's forward (its backward follows suit)
        F.BN_SYNC = self.bn_sync           # ... and by every batch norm's
        if self.is_pn:
            return self.model_fn(pc, is_training, bn_decay=self.bn_decay)
        return self.model_fn(pc, is_training, is_training, self.k, bn_decay=self.bn_decay)

    # -- :206-268 -----------------------------------------------------------------------------
    def forward(self, element, is_training=True):
        """element: dict like the reference's `next_element` (device tensors):
        visiblePoints [B,>=N,3], visiblePoints_org [B,>=4N,3], translation [B,3],
        axisangle [B,3], class_id [B] int64, optional noise [B,N,3]."""
        N = self.NUM_POINT
        vis = element['visiblePoints'].contiguous()
        B, P, _ = vis.shape
        require(P >= N, "visiblePoints has fewer rows than num_point")
        noise = element.get('noise')
        # (from the plan's arena while a step is recorded: the recorded calls keep these addresses)
        pc = _lib.empty((B, N, 3 + NUM_CLASS), dtype=torch.float32, device=vis.device)
        element_mean = _lib.empty((B, 3), dtype=torch.float32, device=vis.device)
        noisy = _lib.empty((B, N, 3), dtype=torch.float32, device=vis.device)
        cls = element['class_id'].to(torch.int64).contiguous()
        if noise is None and is_training:
            # tf.random.normal(shape, stddev=0.004/3), :217, drawn inside the assembly kernel: a function of
            # (this rank's seed, the kernel's own draw counter, cloud, point) -- fresh at every step, also when a
            # recorded step is replayed, independent of the global-step variable (as the reference's generator
            # is), and no generator kernel in front of the step
            _lib.check(_lib.lib().cloudaae_input_assemble_noise(B, P, N, NUM_CLASS, ptr(vis), ptr(cls), ptr(pc),
                                                                ptr(element_mean), ptr(noisy), NOISE_STDDEV,
                                                                self.noise_seed, ptr(self.noise_draws), stream()),
                       "cloudaae_input_assemble_noise")
        else:
            _lib.check(_lib.lib().cloudaae_input_assemble(B, P, N, NUM_CLASS, ptr(vis),
                                                          ptr(noise.contiguous()) if noise is not None else None,
                                                          ptr(cls), ptr(pc), ptr(element_mean), ptr(noisy), stream()),
                       "cloudaae_input_assemble")
        org = element['visiblePoints_org']
        # :214 -- a slice, so fewer than 4N rows pass through here (and fail in chamfer_loss.py:12,
        # whose sum needs n == m, exactly as in the reference)
        visiblePoints_org_final = org[:, 0:N * 4, :].contiguous()
        # the on-line synthesis says which rows of the target are distinct points and which are re-draws of them
        # (hidden_point_removal.py:38-43): the nearest-neighbour search then visits the distinct points only.  The two
        # keys must still describe 'visiblePoints_org' as it is here: a pipeline that reorders or perturbs the target
        # after hidden_point_removal_org drops them (a row whose source is not a distinct row comes back as a NaN
        # distance; CLOUDAAE_NN_PREFIX_VERIFY=1 also compares every copy with its original)
        count2 = row_src2 = None
        if element.get('visiblePoints_org_src') is not None and element.get('num_vis_point_org') is not None:
            count2 = element['num_vis_point_org'].to(torch.int64).contiguous()
            row_src2 = element['visiblePoints_org_src'][:, 0:N * 4].to(torch.int32).contiguous()

        # :232-233 -- xyz_recon = recon_res + mean, trans_pred = trans_res + mean: offered to the fully connected
        # stack: the output layers of the chains the MODEL declares as point outputs (point_outputs: decoder and
        # translation head) add the row vector in their own epilogue when they run as grouped launches
        # (tf_util.fully_connected_chains takes the offer and clears it; a model that declares nothing, or whose
        # decoder emits vectors of another width, leaves it and the additions below run)
        F.FC_OUT_ADD = element_mean
        try:
            xyz_recon_res, rot_pred, trans_pred_res, endpoint = self._call_model(pc, is_training)
        finally:
            folded, F.FC_OUT_ADD = F.FC_OUT_ADD is None, None
        if folded:
            xyz_recon, trans_pred = xyz_recon_res, trans_pred_res
        else:
            xyz_recon = F.AddRowVecFn.apply(xyz_recon_res, element_mean)                          # :232
            trans_pred = F.AddRowVecFn.apply(trans_pred_res.unsqueeze(1), element_mean).squeeze(1)  # :233
        # :236-268 -- Chamfer loss, translation error, SO(3) error (float64) and the weighted total: the search and
        # ONE tail launch (same arithmetic as chamfer_loss.get_loss / trans_distance.get_translation_error /
        # angular_distance_taylor.get_rotation_error / the sum of :268, which stay available on their own)
        trans_label, rot_label, equiv = element['translation'], element['axisangle'], {}
        if self.symmetries is not None:
            from .utils.pose_equiv import nearest_equivalent_pose
            near = nearest_equivalent_pose(rot_pred, rot_label, trans_label, cls, self.symmetries)
            trans_label, rot_label = near['trans_equiv'], near['rot_equiv']
            equiv = dict(axisangle_equiv=rot_label, translation_equiv=trans_label, symmetry_member=near['member'],
                         symmetry_phi=near['phi'])
        (total_loss, xyz_loss, xyz_loss_per_sample, trans_loss, trans_loss_perSample, axag_loss,
         axag_loss_perSample) = F.StepLossFn.apply(xyz_recon, visiblePoints_org_final, trans_pred, trans_label,
                                                   rot_pred, rot_label, *LOSS_WEIGHTS,
                                                   self._one if is_training else None, count2, row_src2)
        return dict(equiv, total_loss=total_loss, xyz_loss=xyz_loss, trans_loss=trans_loss, axag_loss=axag_loss,
                    xyz_recon=xyz_recon, xyz_loss_per_sample=xyz_loss_per_sample,
                    trans_loss_perSample=trans_loss_perSample, axag_loss_perSample=axag_loss_perSample,
                    rot_pred=rot_pred, trans_pred=trans_pred, visiblePoints_final=noisy,
                    visiblePoints_org_final=visiblePoints_org_final, class_id=cls, input_pc=pc,
                    element_mean=element_mean, end_points=endpoint)

    # -- one iteration of the loop at :344-368 ------------------------------------------------
    def train_step(self, element):
        if self.replay:
            return self._planned_step(element)
        return self._step(element)

    def _step(self, element):
        L = _lib.lib()
        s = stream()
        # gradients of the fully connected stack are stored whole by its grouped kernels (batch <= 128):
        # only the encoder's slots (split-K products add into them) are cleared
        self.store.begin_step(zero_grads=True, zero_limit=self._zero_limit)
        if self.bn_sync is not None:
            self.bn_sync.begin_step()
        # self.bn_decay holds min(0.99, 1 - 0.5 * 0.5^floor(batch*BATCH_SIZE/40)) (:194-202) for THIS step: the
        # previous step's optimiser kernel derived it when it advanced `batch` (refresh_bn_decay() after
        # setting `batch` by hand)
        # weight-gradient products of the per-point layers and the reverse neighbour lists run on the
        # library's low-priority side stream (F.SIDE_STREAM) and are joined before anyone reads a gradient
        side = _lib.side_stream() if self.side_stream else None
        F.SIDE_STREAM = side
        F.SIDE_EDGE = os.environ.get("CLOUDAAE_SIDE_STREAM", "0") != "agg"
        F.SIDE_AGG = os.environ.get("CLOUDAAE_SIDE_STREAM", "0") != "edge"
        try:
            out = self.forward(element, is_training=True)
            out['total_loss'].backward(self._one)
            F.flush_deferred_dw()          # (deferred weight-gradient products of layers whose group stayed incomplete)
        finally:
            F.SIDE_STREAM = None
            F.drop_deferred_dw()           # (a step that raised must not leave its jobs to the next one)
        if self.bn_sync is not None:
            self.bn_sync.check()           # an exception inside the all-reduce callback surfaces here, as itself
        if side is not None:
            _lib.stream_wait(stream(), side)
        # RCCL all-reduce of the flat gradient buffer (no-op for 1 rank); bench.py brackets it with HIP events on
        # the compute stream (F.TIMED_SITES["exchange"]): what the step WAITS for, the early piece having travelled
        # behind backward
        rec = F.TIMED_SITES.get("exchange") if self.exchange.active else None
        if rec is not None:
            _lib.host(F._mark, rec)
        _lib.host(self.exchange.finish)
        if rec is not None:
            _lib.host(F._mark, rec)
        n = self.store.flat_params.numel()
        scale = self.exchange.scale
        if self.OPTIMIZER == 'adam':      # tf.train.AdamOptimizer(learning_rate), :266
            # ... whose last workgroup also advances the beta powers and global_step (`batch`) and derives
            # the next step's bn_decay
            _lib.check(L.cloudaae_adam_tf_step(n, ptr(self.store.flat_params), ptr(self.store.flat_grads),
                                               ptr(self.adam_m), ptr(self.adam_v), self.BASE_LEARNING_RATE, 0.9,
                                               0.999, 1e-8, ptr(self.beta1_power), ptr(self.beta2_power), scale,
                                               ptr(self.batch), 1.0, float(self.BATCH_SIZE), BN_INIT_DECAY,
                                               BN_DECAY_DECAY_STEP, BN_DECAY_DECAY_RATE, BN_DECAY_CLIP,
                                               ptr(self.bn_decay), ptr(self._adam_ticket), stream()),
                       "cloudaae_adam_tf_step")
        else:                             # GradientDescentOptimizer(learning_rate*10), :264
            _lib.check(L.cloudaae_sgd(n, ptr(self.store.flat_params), ptr(self.store.flat_grads),
                                      self.BASE_LEARNING_RATE * 10, scale, stream()), "cloudaae_sgd")
            _lib.check(L.cloudaae_increment(ptr(self.batch), 1.0, stream()), "cloudaae_increment")  # global_step
            self.refresh_bn_decay()
        return out

    def refresh_bn_decay(self):
        """bn_decay = min(0.99, 1 - 0.5 * 0.5^floor(batch*BATCH_SIZE/40)) (:194-202) from the current `batch`."""
        _lib.check(_lib.lib().cloudaae_bn_decay_schedule(ptr(self.batch), float(self.BATCH_SIZE), BN_INIT_DECAY,
                                                         BN_DECAY_DECAY_STEP, BN_DECAY_DECAY_RATE, BN_DECAY_CLIP,
                                                         ptr(self.bn_decay), stream()), "cloudaae_bn_decay_schedule")

    # -- the same iteration, recorded once and replayed -----------------------------------------
    def _stage_inputs(self, element):
        """Copy the element into the plan's fixed input buffers (the recorded calls hold their
        addresses); draws the noise of :217 unless the element brings its own."""
        N = self.NUM_POINT
        src = {'visiblePoints': element['visiblePoints'],
               'visiblePoints_org': element['visiblePoints_org'][:, 0:N * 4, :],
               'translation': element['translation'], 'axisangle': element['axisangle'],
               'class_id': element['class_id']}
        dtypes = {'visiblePoints': torch.float32, 'visiblePoints_org': torch.float32,
                  'translation': torch.float32, 'axisangle': torch.float64, 'class_id': torch.int64,
                  'num_vis_point_org': torch.int64, 'visiblePoints_org_src': torch.int32}
        if element.get('visiblePoints_org_src') is not None and element.get('num_vis_point_org') is not None:
            # (the synthesis' account of which target rows are re-draws: forward() hands it to the Chamfer search)
            src['num_vis_point_org'] = element['num_vis_point_org']
            src['visiblePoints_org_src'] = element['visiblePoints_org_src'][:, 0:N * 4]
        own_noise = element.get('noise') is not None
        key = tuple((k, tuple(v.shape), str(dtypes[k])) for k, v in src.items()) + (('noise', own_noise),)
        if key != self._plan_key:
            # another input shape: park the current recording (up to 4 are kept, e.g. a training and a
            # shorter last batch alternating) and pick up / start the one for this shape
            if self._plan_key is not None and self._plan is not None:
                self._plans[self._plan_key] = (self._plan, self._plan_out, self._static)
                while len(self._plans) > 4:
                    gone = self._plans.pop(next(iter(self._plans)))
                    if self.bn_sync is not None:
                        self.bn_sync.forget(gone[0])
            self._staged = None
            self._plan_key = key
            if key in self._plans:
                self._plan, self._plan_out, self._static = self._plans.pop(key)
            else:
                self._plan = self._plan_out = None
                self._static = {k: torch.empty(tuple(v.shape), dtype=dtypes[k], device=self.device)
                                for k, v in src.items()}
                if own_noise:       # (otherwise the assembly kernel draws it: nothing to stage)
                    B = src['visiblePoints'].shape[0]
                    self._static['noise'] = torch.empty((B, N, 3), dtype=torch.float32, device=self.device)
        # reuse_staged_inputs (off by default): the caller promises that passing the very same tensor
        # objects again means the same contents (a fixed batch, as in bench.py) -- then they are not
        # copied again.  It cannot be detected safely: kernels that fill a tensor through its raw
        # pointer do not bump torch's version counter.
        seen = self._staged if (self.reuse_staged_inputs and self._staged is not None) else {}
        staged = {}
        for k, v in src.items():
            base = element[k]
            staged[k] = base
            if seen.get(k) is not base:
                self._static[k].copy_(v, non_blocking=True)
        if own_noise:
            staged['noise'] = element['noise']
            if seen.get('noise') is not element['noise']:
                self._static['noise'].copy_(element['noise'])
        self._staged = staged
        return self._static

    def _planned_step(self, element):
        self._set_mode()                   # (a replay reads the library's knob at every recorded call)
        static = self._stage_inputs(element)
        if self._plan is None:
            plan = _lib.StepPlan(self.device)
            with _lib.record(plan):
                out = self._step(static)
            if plan.foreign_ops:
                # something in this configuration still runs as a torch kernel: such a step cannot
                # be re-issued faithfully, so this graph keeps stepping the ordinary way
                import warnings
                warnings.warn("step not replayable (torch kernels inside: %s); running eagerly"
                              % sorted(set(plan.foreign_ops)))
                self.replay = False
                return out
            self._plan = plan
            self._plan_out = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
            return self._plan_out
        self._plan.replay()
        return self._plan_out

    def eval_step(self, element):
        with torch.no_grad():
            return self.forward(element, is_training=False)

    # -- tf.train.Saver (:276, :418-424): every variable under its TF name ---------------------
    def checkpoint(self, name_scope=EMA_NAME_SCOPE):
        """name -> numpy array, with the names tf.train.Saver writes for this graph: the model variables, the BN
        moving averages (`<scope>/bn/<name_scope>/<scope>/bn/moments/Squeeze[_1]/ExponentialMovingAverage`: TF names
        an EMA shadow after the op it shadows, and the model is built under tf.name_scope('decoder'), :223 -- the
        shipped snapshot and evaluate_cloudAAE_ycbv.py:436 use '6d_pose'), the Adam slots `<var>/Adam`,
        `<var>/Adam_1`, `beta1_power`, `beta2_power`, and the step counter `Variable` (:192)."""
        ck = {tf_variable_name(n, name_scope): t.cpu().numpy() for n, t in self.store.state_dict().items()}
        for v in self.store.trainable_variables():
            o = self.store.offsets[v.name]
            n = v.data.numel()
            ck[v.name + '/Adam'] = self.adam_m[o:o + n].view(v.shape).cpu().numpy()
            ck[v.name + '/Adam_1'] = self.adam_v[o:o + n].view(v.shape).cpu().numpy()
        ck['beta1_power'] = self.beta1_power.cpu().numpy().reshape(())
        ck['beta2_power'] = self.beta2_power.cpu().numpy().reshape(())
        ck['Variable'] = self.batch.cpu().numpy().reshape(())
        return ck

    def save(self, path, fmt='npz', name_scope=EMA_NAME_SCOPE):
        """saver.save(sess, path) (:424), by rank 0.  fmt 'npz': a NumPy archive `path`.npz; fmt 'tf': a TensorFlow
        V2 checkpoint `path`.index + `path`.data-00000-of-00001 (tf_checkpoint.py) that tf.train.Saver restores."""
        import numpy as np
        require(fmt in ('npz', 'tf'), "fmt must be 'npz' or 'tf'")
        if fmt == 'tf':
            if self.rank == 0:
                from . import tf_checkpoint
                tf_checkpoint.write_checkpoint(path, self.checkpoint(name_scope))
            return path
        if self.rank == 0:
            tmp = path + '.tmp.npz'
            np.savez(tmp, **self.checkpoint(name_scope))
            os.replace(tmp, path + '.npz')
        return path + '.npz'

    def restore(self, path, strict=True):
        """saver.restore(sess, path) (:425-430; evaluate_cloudAAE_ycbv.py:495-499): a TensorFlow V2 checkpoint
        prefix (`path`.index exists -- e.g. the reference's trained_network/<run>/model.ckpt), or what save() wrote,
        or any name -> array archive with the reference's variable names (optimizer slots optional).  BN moving
        averages are accepted under any name scope ('decoder', '6d_pose', none)."""
        import numpy as np
        if os.path.exists(path + '.index') or path.endswith('.index'):
            from . import tf_checkpoint
            ck = tf_checkpoint.load_checkpoint(path)
        else:
            with np.load(path if path.endswith('.npz') else path + '.npz') as z:
                ck = {k: z[k] for k in z.files}
        ck = {store_variable_name(k): v for k, v in ck.items()}
        names = set(self.store.vars)
        self.store.load_state_dict({k: v for k, v in ck.items() if k in names}, strict=strict)
        with torch.no_grad():
            for v in self.store.trainable_variables():
                o = self.store.offsets[v.name]
                n = v.data.numel()
                for slot, flat in (('/Adam', self.adam_m), ('/Adam_1', self.adam_v)):
                    if v.name + slot in ck:
                        flat[o:o + n].copy_(torch.as_tensor(ck[v.name + slot], dtype=torch.float32).reshape(-1))
            for key, t in (('beta1_power', self.beta1_power), ('beta2_power', self.beta2_power), ('Variable', self.batch)):
                if key in ck:
                    t.fill_(float(ck[key]))
        self.refresh_bn_decay()      # the decay of the next step follows the restored global_step


_EMA_STORE = re.compile(r'^(.*)/bn/moments/(Squeeze(?:_1)?)/ExponentialMovingAverage$')
_EMA_TF = re.compile(r'^(.*)/bn/(?:[^/]+/)?\1/bn/moments/(Squeeze(?:_1)?)/ExponentialMovingAverage$')


def tf_variable_name(name, name_scope=EMA_NAME_SCOPE):
    """The name tf.train.Saver gives a variable of the store: only the BN moving averages differ -- TF names an
    EMA shadow `<variable scope>/<full name of the shadowed op>/ExponentialMovingAverage` and that op lives in the
    name scope the model was built under."""
    m = _EMA_STORE.match(name)
    if m is None or not name_scope:
        return name
    return '%s/bn/%s/%s/bn/moments/%s/ExponentialMovingAverage' % (m.group(1), name_scope, m.group(1), m.group(2))


def store_variable_name(name):
    """Inverse of tf_variable_name for any name scope."""
    m = _EMA_TF.match(name)
    if m is None:
        return name
    return '%s/bn/moments/%s/ExponentialMovingAverage' % (m.group(1), m.group(2))


# ---- the data pipeline of train_cloudAAE_ycbv.py:42-117, batched on the GPU --------------------
def get_object_model(x, obj_models):
    """:68-76  x['obj_batch'] = obj_models[class_id]  (obj_models [21,2048,6] device tensor); the
    gather itself happens inside transform_object_model."""
    x['obj_model'] = obj_models
    return x


def get_rotation_matrix(x):
    """:79-85  rot_mat = float32(exponential_map(float64(axisangle)))."""
    x['axisangle'] = x['axisangle'].to(torch.float64)
    x['rot_mat64'] = angular_distance_taylor.exponential_map(x['axisangle'])
    x['rot_mat'] = x['rot_mat64'].to(torch.float32)
    return x


def transform_object_model(x):
    """:88-93  model_xyz_rot_trans = obj_batch[:, :, 0:3] R^T + translation."""
    models = x['obj_model'].to(torch.float32).contiguous()
    nmodels, npts, _ = models.shape
    t = x['translation'].to(torch.float32).contiguous()
    B = t.shape[0]
    out = torch.empty((B, npts, 3), dtype=torch.float32, device=t.device)
    cls = x['class_id'].to(torch.int64).contiguous()
    _lib.check(_lib.lib().cloudaae_transform_object_model(B, npts, nmodels, ptr(models), ptr(cls),
                                                          ptr(x['rot_mat64'].contiguous()), ptr(t), ptr(out),
                                                          stream()), "cloudaae_transform_object_model")
    x['model_xyz_rot_trans'] = out
    return x


def get_small_data(records, obj_models, seed=0, rows=None, rows_org=None, occluder='spherical', dataset='ycbv',
                   first_index=0, occluder_seed=None, visibility='hpr', rendered=None):
    """:96-117 for one batch: records = dict of device tensors translation [B,3], axisangle [B,3],
    class_id [B] (e.g. from tfrecord_io.PoseRecords.epoch); returns the reference's element dict:
    visiblePoints [B,2449,3], visiblePoints_org [B,2049,3], occluder, model_xyz_rot_trans, ...
    rows / rows_org: other row counts of visiblePoints / visiblePoints_org (default: the reference's model points
    [+ occluder points] + 1), filled by the reference's rule -- visible points, then random re-draws of visible
    points (hidden_point_removal.py:38-40).  BASELINE configs[4] (N = 4096) needs a Chamfer target of 4N = 16384 rows,
    more than any model has points.
    occluder: 'spherical' (two Gaussian blobs, 400 points) or 'object' (512 points of a class model rotated by the sample's
    rotation, generate_occluder.py:5-35: visiblePoints then has 2048 + 512 + 1 rows); dataset: the camera constants of
    either.  The object occluder of sample i is a function of (occluder_seed, first_index + i) -- occluder_seed defaults
    to `seed`.  The defaults give what this function gave before it had these arguments, bit for bit.
    visibility: 'hpr' (the above) or 'rendered': the clouds come from rendered depth frames of the sample's mesh behind a
    mesh occluder (utils/rendered_data.rendered_element, which `rendered` holds the keyword arguments of: packed_meshes,
    num_point, and optionally mesh_index, sensor, sensor_seed, height, width, min_visible); the records must bring
    rot_mat64 (sampled poses do), obj_models, rows, rows_org and occluder are not used, and the sample is a function of
    (occluder_seed, first_index + i)."""
    require(visibility in ('hpr', 'rendered'), "visibility must be 'hpr' or 'rendered'")
    if visibility == 'rendered':
        from .utils import rendered_data
        require(rendered is not None and rendered.get('packed_meshes') is not None and rendered.get('num_point'),
                "visibility='rendered' needs rendered=dict(packed_meshes=..., num_point=...)")
        require(records.get('rot_mat64') is not None, "visibility='rendered' needs sampled poses (rot_mat64)")
        kw = dict(rendered)
        return rendered_data.rendered_element(records, kw.pop('packed_meshes'), kw.pop('mesh_index', None),
                                              kw.pop('num_point'), seed if occluder_seed is None else occluder_seed,
                                              first_index, dataset=dataset, **kw)
    from .utils import generate_occluder, hidden_point_removal as hpr
    require(occluder in ('spherical', 'object'), "occluder must be 'spherical' or 'object'")
    x = dict(records)
    x = get_object_model(x, obj_models)
    if x.get('rot_mat64') is None:
        x = get_rotation_matrix(x)
    else:                                 # sampled poses bring the exponential map of their axis-angle along
        x['rot_mat'] = x['rot_gen_mat'] if x.get('rot_gen_mat') is not None else x['rot_mat64'].to(torch.float32)
    x = transform_object_model(x)
    if occluder == 'object':
        x = generate_occluder.get_random_object_occluder(x, obj_models.shape[0], dataset=dataset, first_index=first_index,
                                                         seed=seed if occluder_seed is None else occluder_seed)
    else:
        x = generate_occluder.get_random_spherical_occluder(x, dataset, seed=seed)
    x = hpr.sphericalFlip(x, None, 0.8 * math.pi)            # center = zeros_like(translation), :103
    x = hpr.hidden_point_removal(x, seed=seed, rows=rows)
    x = hpr.sphericalFlip_org(x, None, 0.8 * math.pi)
    x = hpr.hidden_point_removal_org(x, seed=seed, rows=rows_org)
    return x


def synthetic_element(local_batch, num_point, device, seed=123456789, rank=0, single_class=None):
    """Synthetic `next_element` of SURVEY.md section 8d, generated on the device: object-scale
    points N(0, 0.05^2) + translation (t_xy ~ U(+-0.25), t_z ~ U(0.5,1.5)), class ids U{0..20},
    axis-angle = uniform axis x U(-pi,pi); the target cloud has 4N points of the same law."""
    g = torch.Generator(device=device)
    g.manual_seed(seed + rank)
    B, N = local_batch, num_point
    t = torch.empty((B, 3), device=device)
    t[:, :2] = torch.rand((B, 2), generator=g, device=device) * 0.5 - 0.25
    t[:, 2] = torch.rand((B,), generator=g, device=device) + 0.5
    vis = torch.randn((B, N, 3), generator=g, device=device) * 0.05 + t[:, None, :]
    org = torch.randn((B, 4 * N, 3), generator=g, device=device) * 0.05 + t[:, None, :]
    cls = torch.randint(0, NUM_CLASS, (B,), generator=g, device=device)
    if single_class is not None:
        cls[:] = single_class
    axis = torch.randn((B, 3), generator=g, device=device, dtype=torch.float64)
    axis = axis / axis.norm(dim=1, keepdim=True)
    angle = (torch.rand((B,), generator=g, device=device, dtype=torch.float64) * 2 - 1) * math.pi
    return dict(visiblePoints=vis, visiblePoints_org=org, class_id=cls, translation=t.clone(),
                axisangle=axis * angle[:, None])


def synthetic_object_models(num_models=NUM_CLASS, num_point=2048, seed=123456789, device=None):
    """Stand-ins for object_model_tfrecord/obj_models.tfrecords (train...:42-54: 21 x [2048, 6] xyz + rgb) with any
    number of points per model -- BASELINE configs[4] feeds N = 4096 input points, more than the shipped models'
    2048: points on closed surfaces of YCB-like extent (superellipsoids of half-axes 0.03 ... 0.11 m, exponent
    0.6 ... 2.5: from box-like to rounded), rgb = normalised position."""
    g = torch.Generator().manual_seed(seed)
    out = torch.empty((num_models, num_point, 6), dtype=torch.float32)
    for m in range(num_models):
        half = torch.rand(3, generator=g) * 0.08 + 0.03
        e = float(torch.rand((), generator=g) * 1.9 + 0.6)
        d = torch.randn((num_point, 3), generator=g)
        d = d / d.norm(dim=1, keepdim=True)
        r = (d.abs() ** (2.0 / e)).sum(1, keepdim=True) ** (-e / 2.0)      # |x/a|^(2/e) + ... = 1 along direction d
        out[m, :, :3] = d * r * half
        out[m, :, 3:] = d * 0.5 + 0.5
    return out if device is None else out.to(device)


class SampledPoses(object):
    """The stand-in for tfrecord_io.PoseRecords when poses are drawn instead of read: `epoch()` yields device dicts from
    utils.sample_pose_in_frustum.sample_poses.  Sample i of this rank's batch of step s is global sample
    g = s * global_batch + rank * local_batch + i (s counts from the first epoch on): every rank draws its own index
    range, nothing is sharded, and a run of other batch or world size meets the same samples at the same g."""

    def __init__(self, epoch_size, global_batch, rank=0, world=1, seed=123456789, classes=None, dataset='ycbv',
                 camera=None, device=None, num_models=NUM_CLASS):
        require(global_batch % world == 0, "global batch must divide by the number of ranks")
        self.epoch_size, self.global_batch, self.rank, self.world = int(epoch_size), int(global_batch), int(rank), int(world)
        self.local_batch = self.global_batch // self.world
        self.seed, self.classes, self.dataset, self.camera = int(seed), classes, dataset, camera
        self.device, self.num_models = device, int(num_models)

    def __len__(self):                     # samples this rank sees per epoch
        return self.steps_per_epoch() * self.local_batch

    def steps_per_epoch(self):
        return self.epoch_size // self.global_batch

    def first_index(self, epoch, batch_idx):
        return (epoch * self.steps_per_epoch() + batch_idx) * self.global_batch + self.rank * self.local_batch

    def epoch(self, batch_size, epoch=0):
        from .utils import sample_pose_in_frustum as spf
        require(batch_size == self.local_batch, "SampledPoses was built for another local batch")
        for batch_idx in range(self.steps_per_epoch()):
            g0 = self.first_index(epoch, batch_idx)
            rec = spf.sample_poses(batch_size, self.seed, g0, classes=self.classes, dataset=self.dataset,
                                   camera=self.camera, device=self.device, num_models=self.num_models)
            rec['first_index'] = g0
            yield rec


class ClassLossLog(object):
    """The per-class running averages of :318-321 / :397-414 (what the reference sends to
    TensorBoard every 1000 batches), accumulated on the device so the loop never syncs."""

    def __init__(self, device):
        self.sums = torch.zeros((3, NUM_CLASS), dtype=torch.float64, device=device)
        self.count = torch.zeros((NUM_CLASS,), dtype=torch.float64, device=device)
        self.total = torch.zeros((NUM_CLASS,), dtype=torch.int64, device=device)

    def add(self, out):
        cls = out['class_id']
        B = cls.shape[0]       # xyz_loss_per_sample is per point [B,4N] (chamfer_loss.py:12); np.average(:399) flattens it
        per = torch.stack([out[k].detach().double().reshape(B, -1).mean(1)
                           for k in ('xyz_loss_per_sample', 'axag_loss_perSample', 'trans_loss_perSample')])
        self.sums.index_add_(1, cls, per)
        self.count.index_add_(0, cls, torch.ones_like(cls, dtype=torch.float64))

    def flush(self):
        """-> list of (class, n_total, xyz, axag, trans) for classes seen since the last flush."""
        self.total += self.count.long()
        sums, count, total = self.sums.cpu(), self.count.cpu(), self.total.cpu()
        rows = [(c, int(total[c]), float(sums[0, c] / count[c]), float(sums[1, c] / count[c]),
                 float(sums[2, c] / count[c])) for c in range(NUM_CLASS) if count[c] > 0]
        self.sums.zero_()
        self.count.zero_()
        return rows


def train_graph(graph, records, obj_models, epoch, class_log=None, log=None, logdir=None, seed=None,
                max_batches=None, print_every=1, summary_every=1000, occluder='spherical', dataset='ycbv',
                visibility='hpr', rendered=None):
    """One epoch of the reference's train_graph (:332-437): draw shuffled batches of pose records,
    synthesise the element on the GPU (get_small_data), train_step, per-class loss bookkeeping
    every `summary_every` batches, checkpoint at the end of the epoch (:418-424).
    `records` is this rank's tfrecord_io.PoseRecords shard, or a SampledPoses (poses drawn on the GPU: nothing is read
    on the host or copied); obj_models the [21,2048,6] device tensor.  visibility, rendered: get_small_data's ('rendered'
    needs a SampledPoses)."""
    require(visibility == 'hpr' or isinstance(records, SampledPoses), "visibility='rendered' needs sampled poses")
    start = time.time()
    dev = graph.device
    batch_idx = 0
    out = None
    sampled = isinstance(records, SampledPoses)
    batches = records.epoch(graph.local_batch, epoch) if sampled else records.epoch(graph.local_batch, seed=seed)
    for rec in batches:
        if max_batches is not None and batch_idx >= max_batches:
            break
        batch_seed = (epoch << 32) + batch_idx * graph.world + graph.rank
        if sampled:
            element = get_small_data(rec, obj_models, seed=batch_seed, occluder=occluder, dataset=dataset,
                                     first_index=rec['first_index'], occluder_seed=records.seed, visibility=visibility,
                                     rendered=rendered)
        else:
            element = get_small_data({k: torch.as_tensor(v).to(dev, non_blocking=True) for k, v in rec.items()},
                                     obj_models, seed=batch_seed, occluder=occluder, dataset=dataset)
        out = graph.train_step(element)
        if class_log is not None:
            class_log.add(out)
        if log is not None and print_every and batch_idx % print_every == 0:
            log("epoch %d batch %d xyz_loss %f trans_loss %f axag_loss %f"
                % (epoch, batch_idx, float(out['xyz_loss'].detach()), float(out['trans_loss'].detach()),
                   float(out['axag_loss'].detach())))
        if class_log is not None and log is not None and batch_idx != 0 and batch_idx % summary_every == 0:
            for c, n, xyz, axag, trans in class_log.flush():
                log("  class %2d samples %8d xyz_loss %f axag_loss %f trans_loss %f" % (c, n, xyz, axag, trans))
        batch_idx += 1
    torch.cuda.synchronize(dev)
    if log is not None:
        log('End of data!')
    if logdir is not None:
        name = "model_%d.ckpt" % epoch if (epoch + 1) % 50 == 0 else "model.ckpt"       # :419-422
        path = graph.save(os.path.join(logdir, name))
        if log is not None and graph.rank == 0:
            log("Model saved in file: %s" % path)
    if log is not None:
        log('Current epoch Time elapsed %.1f s (%d batches)' % (time.time() - start, batch_idx))
    return batch_idx, out


def load_object_models(data_dir, device):
    """object_model_tfrecord/obj_models.tfrecords under `data_dir` -> device tensor [21,2048,6]."""
    from . import tfrecord_io
    models, _ = tfrecord_io.read_and_decode_obj_model(os.path.join(data_dir, "object_model_tfrecord", "obj_models.tfrecords"))
    return torch.as_tensor(models).to(device)


def load_dataset(data_dir, device, rank=0, world=1, classes=None):
    """The files of :31-39 under `data_dir`: object models -> device tensor [21,2048,6];
    pose records of the chosen classes -> this rank's shard."""
    from . import tfrecord_io
    models, _ = tfrecord_io.read_and_decode_obj_model(os.path.join(data_dir, "object_model_tfrecord", "obj_models.tfrecords"))
    obj_models = torch.as_tensor(models).to(device)
    classes = range(NUM_CLASS) if classes is None else classes
    files = [os.path.join(data_dir, "ycb_video_data_tfRecords", "train_syn", "%d_syn.tfrecords" % c) for c in classes]
    records = tfrecord_io.PoseRecords(files)
    return obj_models, (records.shard(rank, world) if world > 1 else records)


def symmetry_table_for(spec, obj_models, classes=None, meshes='', mesh_scale=1.0, device=None):
    """--symmetries auto|FILE -> (pose_equiv.SymmetryTable over the obj_models.shape[0] classes, the lines that say what
    was found).  auto: symmetries_of_meshes of the --meshes when there are any, else symmetries_of_models of the class
    models, for `classes` (default: all)."""
    import json
    from .utils import pose_equiv, symmetry
    num_class = int(obj_models.shape[0])
    if spec != 'auto':
        with open(spec) as f:
            entries = json.load(f)["classes"]
        ids = [int(e["class"]) for e in entries]
        return pose_equiv.load_symmetry_table(spec, num_class, device), symmetry.kind_lines(entries, ids)
    ids = list(range(num_class)) if classes is None else [int(c) for c in classes]
    if meshes:
        from .utils import mesh_models
        files = mesh_models.mesh_files(meshes)
        results = symmetry.symmetries_of_meshes([files[c] for c in ids], scale=mesh_scale, device=device, mesh_ids=ids)
    else:
        results = symmetry.symmetries_of_models(obj_models[ids][:, :, :3].contiguous())
    table = pose_equiv.SymmetryTable.from_results(results, num_class, ids, device)
    return table, symmetry.kind_lines(results, ids)


def main(argv=None):
    parser = get_training_argparser()
    groups = parse_arg_groups(parser, argv)
    general, topts, hyper, extra = groups['general'], groups['training_options'], groups['hyperparameters'], groups['mi355x']
    if extra['meshes'] and extra['poses'] != 'sampled':
        parser.error("--meshes needs --poses sampled (pose records belong to the shipped object models)")
    if extra['visibility'] == 'rendered' and not (extra['meshes'] and extra['poses'] == 'sampled'):
        parser.error("--visibility rendered needs --poses sampled and --meshes (the frames are rendered from the meshes)")
    if extra['sensor'] != 'none' and extra['visibility'] != 'rendered':
        parser.error("--sensor needs --visibility rendered (there is no depth frame to apply it to otherwise)")
    if extra['symmetries'] != 'none' and not (extra['data_dir'] or extra['poses'] == 'sampled'):
        parser.error("--symmetries needs object models: give --data_dir or --poses sampled")
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        local = int(os.environ.get('LOCAL_RANK', '0'))
        torch.cuda.set_device(local)
        dist.init_process_group('nccl')
        general['gpu'] = local
    graph = TrainGraph(general, topts, hyper, model_fn=extra['model_fn'], k_neighbor=extra['k'], replay=True,
                       gemm_dtype=extra['gemm_dtype'], deterministic=bool(extra.get('deterministic')))
    if extra['restore']:
        graph.restore(extra['restore'])
    classes = [int(c) for c in extra['classes'].split(',') if c != ''] or None
    sampled = extra['poses'] == 'sampled'
    if extra['data_dir'] or sampled:
        # the reference's run: LOG_DIR/<NUM_CLASS>/6d/<timestamp>/log_train.txt (:150-157)
        logdir = os.path.join(general['log_dir'], str(NUM_CLASS), "6d", time.strftime("%Y%m%d-%H%M%S"))
        fout = None
        if graph.rank == 0:
            os.makedirs(logdir, exist_ok=True)
            fout = open(os.path.join(logdir, 'log_train.txt'), 'w')
            for d in (general, topts, hyper):
                fout.write(str(d) + '\n')

        def log(msg):
            if graph.rank == 0:
                fout.write(msg + '\n')
                fout.flush()
                print(msg)
        if sampled:
            # poses drawn on the GPU: only the object models are read (or made up, without --data_dir); every rank draws
            # its own range of global sample indices
            if extra['meshes']:
                # the models come from the meshes (every rank builds the same ones: a function of the seed and the
                # file's position), and there are as many classes as files
                from .utils import mesh_models
                obj_models = mesh_models.models_from_meshes(mesh_models.mesh_files(extra['meshes']),
                                                            scale=extra['mesh_scale'], device=graph.device)
            else:
                obj_models = load_object_models(extra['data_dir'], graph.device) if extra['data_dir'] \
                    else synthetic_object_models(device=graph.device)
            records = SampledPoses(extra['epoch_size'], graph.BATCH_SIZE, graph.rank, graph.world, seed=extra['pose_seed'],
                                   classes=classes, dataset=extra['dataset'], device=graph.device,
                                   num_models=obj_models.shape[0])
        else:
            obj_models, records = load_dataset(extra['data_dir'], graph.device, graph.rank, graph.world, classes=classes)
        rendered = None
        if extra['visibility'] == 'rendered':
            from .utils import mesh_models
            rendered = dict(packed_meshes=mesh_models.pack_meshes(mesh_models.mesh_files(extra['meshes']),
                                                                  extra['mesh_scale'], graph.device),
                            num_point=graph.NUM_POINT, sensor=None if extra['sensor'] == 'none' else extra['sensor'],
                            sensor_seed=extra['sensor_seed'])
        log("%d pose records on rank 0, %d batches per epoch" % (len(records), len(records) // graph.local_batch))
        if extra['symmetries'] != 'none':
            table, lines = symmetry_table_for(extra['symmetries'], obj_models, classes, extra['meshes'], extra['mesh_scale'],
                                              graph.device)
            graph.set_symmetries(table)
            for line in lines:
                log(line)
        class_log = ClassLossLog(graph.device)
        for epoch in range(int(topts['max_epoch'])):
            log('**** EPOCH %03d ****' % epoch)
            train_graph(graph, records, obj_models, epoch, class_log, log, logdir, seed=123456789 + epoch,
                        max_batches=extra['steps'] or None, print_every=extra['print_every'],
                        occluder=extra['occluder'], dataset=extra['dataset'], visibility=extra['visibility'],
                        rendered=rendered)
        return
    el = synthetic_element(graph.local_batch, graph.NUM_POINT, graph.device, rank=graph.rank)
    t0 = time.time()
    for i in range(extra['steps'] or 100):
        out = graph.train_step(el)
        if i % 10 == 0 and graph.rank == 0:
            print("step %d xyz_loss %f trans_loss %f axag_loss %f" %
                  (i, float(out['xyz_loss']), float(out['trans_loss']), float(out['axag_loss'])))
    torch.cuda.synchronize()
    if graph.rank == 0:
        print("%.1f clouds/s" % ((extra['steps'] or 100) * graph.BATCH_SIZE / (time.time() - t0)))


if __name__ == "__main__":
    main()
