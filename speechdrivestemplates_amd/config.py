"""Config shim with the reference's keys and merge order (configs/default.py:4-97, main.py:29-33):
defaults <- yaml file <- CLI ``KEY VAL`` pairs, then frozen.  yacs is not a dependency: ``CfgNode`` here is
a ~60-line attribute-access dict with the four methods the reference calls (merge_from_file,
merge_from_list, freeze, clone)."""
import ast
import copy
import math

import yaml

_DEFAULTS = {
    "PIPELINE_TYPE": None,
    "VOICE2POSE": {
        "STRICT_LOADING": True,
        "GENERATOR": {
            "NAME": None, "LEAKY_RELU": True, "NORM": "IN", "LAMBDA_REG": 1.0, "LAMBDA_CLIP_KL": 0.1,
            # extensions (the regression loss on noisy keypoints, ops.RegLossFn / csrc/reg_loss.hip; the defaults are the
            # reference's plain mean, computed by the same kernels as before):
            # LAMBDA_VEL >= 0: weight of G_vel_loss, an L1 on the first differences over time of (prediction - ground truth).
            # REG_MIN_CONFIDENCE: a float c = an element takes part in G_reg_loss (and a pair of frames in G_vel_loss) only where the batch's
            # 'poses_score' (the OpenPose confidence) is > c; each sum is divided by the number of elements that took part.  None masks nothing.
            # REG_PART_WEIGHTS: [body, face, hands], three floats >= 0 that multiply the terms of keypoints 0-8 / 9-78 / 79-120 (not the
            # divisors).  None = 1 everywhere.
            "LAMBDA_VEL": 0.0, "REG_MIN_CONFIDENCE": None, "REG_PART_WEIGHTS": None,
            # extensions (losses on the limbs of the skeleton, ops.BoneLossFn / csrc/bone_loss.hip; off by default = the
            # step as it was), on the de-normalised global keypoints, over the limbs the renderer draws (PoseTransforms.skeleton_edges):
            # LAMBDA_BONE >= 0: weight of G_bone_loss, the mean of |predicted length - true length| / max(true length, BONE_MIN_LENGTH).
            # LAMBDA_BONE_DIR >= 0: weight of G_bone_dir_loss, the mean of 1 - cos between the predicted and the true limb vector.
            # BONE_MIN_LENGTH > 0: the floor (de-normalised pixels) of the divisor of the length term.
            # REG_MIN_CONFIDENCE (a limb is live where both ends, and their part roots, are) and REG_PART_WEIGHTS (a limb takes the
            # weight of its part) apply to both when they are set.
            "LAMBDA_BONE": 0.0, "LAMBDA_BONE_DIR": 0.0, "BONE_MIN_LENGTH": 1.0,
            "CLIP_CODE": {"DIMENSION": None, "LR_SCALING": 1.0, "TRAIN": True, "FRAME_VARIANT": False,
                          "SAMPLE_FROM_NORMAL": False, "TEST_WITH_GT_CODE": False, "EXTERNAL_CODE": False,
                          "EXTERNAL_CODE_PTH": None},
        },
        "POSE_ENCODER": {"NAME": "PoseSeqEncoder", "AE_CHECKPOINT": None},
        "POSE_DISCRIMINATOR": {"NAME": None, "LEAKY_RELU": False, "LAMBDA_GAN": 1.0, "MOTION": True, "WHITE_LIST": None},
    },
    "POSE2POSE": {
        "AUTOENCODER": {"NAME": None, "LEAKY_RELU": True, "NORM": "BN", "CODE_DIM": 32},
        "LAMBDA_REG": 1.0, "LAMBDA_KL": 0.1,
    },
    "DATASET": {
        "NAME": "GestureDataset", "ROOT_DIR": "datasets/speakers", "SUBSET": None, "NUM_LANDMARKS": 121,
        "HIERARCHICAL_POSE": True, "SPEAKER": None, "NUM_FRAMES": 64, "AUDIO_LENGTH": 68267, "MAX_DEMO_LENGTH": 24,
        "AUDIO_SR": 16000, "FPS": 15, "CACHING": False,
        # extension (not in the reference): number of clips of the seeded synthetic dataset used by bench/tests
        "SYNTHETIC_CLIPS": 4096,
        # extension: an npz of DATASET.SPEAKER's statistics (python -m speechdrivestemplates_amd.speaker_stats),
        # registered on every rank before any dataset is built -- the reference's "paste into speakers_stat.py" step.  None: built-in only
        "SPEAKER_STAT_FILE": None,
    },
    "TRAIN": {"NUM_EPOCHS": 100, "BATCH_SIZE": 32, "SAVE_VIDEO": True, "SAVE_NPZ": False, "LR": 1e-4, "WD": 0,
              "LR_SCHEDULER": True, "PRETRAIN_FROM": None, "VALIDATE": True, "NUM_RESULT_SAMPLE": 2,
              "CHECKPOINT_INTERVAL": 1,
              # extensions (optimiser-side safeguards, optim.StepGuard / csrc/optim_guard.hip; all off by default = the
              # step as it was).  Step groups are what optimizer_updates steps together: {optimizerClipCode, optimizerG} and {optimizerD_pose}.
              # GRAD_CLIP_NORM: a positive float clips the global L2 norm of each step group's gradient to it, as
              # torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False) does: coefficient max_norm / (norm + 1e-6), at most 1.
              # SKIP_NONFINITE_STEP True: a step group whose gradient norm is not finite is not applied (parameters, moments, step counter
              # and EMA keep their bits; a device counter goes up).  False: such a gradient makes the parameters NaN, as in torch.
              # Either key also logs grad_norm_G / grad_norm_D (before clipping) and skipped_steps_G / skipped_steps_D with the losses.
              # EMA_DECAY: d in (0, 1) keeps ema = d * ema + (1 - d) * p of the generator-side parameters (optimizerG, optimizerClipCode;
              # pose2pose's optimiser), updated after every applied step and saved as 'model_ema_state_dict'.  The discriminator and the
              # BatchNorm running statistics (buffers) are not averaged.
              "GRAD_CLIP_NORM": None, "SKIP_NONFINITE_STEP": False, "EMA_DECAY": None,
              # extension (audio augmentation inside the train step, augment.Augmenter / csrc/augment.hip; Voice2Pose
              # only; every key off by default = the step as it was, no kernel launched).  With ENABLE the training forward pass hands the
              # batch's audio through one GPU pass before the mel front end and zeroes bands and spans of the power mel behind it; evaluation
              # and the demo hear clean audio.  Everything random is a Philox4x32-10 word of (SEED, global step, clip index): the same on any
              # number of ranks, at any batch size and after a resume.
              # SEED: integer in [0, 2^64), the Philox key.  GAIN_DB G in [0, 40]: a per-clip gain, uniform over 256 levels in [-G, +G] dB.
              # NOISE_SNR_DB: None, or [lo, hi] with -20 <= lo <= hi <= 80: white noise at a per-clip SNR (256 levels in [lo, hi] dB) against
              # the clip's own RMS; NOISE_PROB in [0, 1]: the share of clips that get it.  SHIFT_MS in [0, 500]: the audio moves against the
              # poses by a uniform whole number of samples in +-floor(SHIFT_MS * AUDIO_SR / 1000), zero-filled.  POLARITY: a random sign
              # flip per clip.  MEL_FREQ_MASKS [n, w]: n in 0 .. 4 bands of 0 .. w (at most 40) mel bins set to 0; MEL_TIME_MASKS [n, w]:
              # n in 0 .. 4 spans of 0 .. w (at most 100) mel columns set to 0.
              "AUGMENT": {"ENABLE": False, "SEED": 0, "GAIN_DB": 0.0, "NOISE_SNR_DB": None, "NOISE_PROB": 1.0, "SHIFT_MS": 0.0,
                          "POLARITY": False, "MEL_FREQ_MASKS": [0, 0], "MEL_TIME_MASKS": [0, 0]},
              # extension (pose augmentation inside the train step, pose_augment.PoseAugmenter / csrc/pose_augment.hip; DESIGN.md section 30;
              # Voice2Pose and Pose2Pose; needs DATASET.NUM_LANDMARKS 121; off by default = the step as it was, no kernel launched, the code
              # tables as large as they were).  With ENABLE the training forward pass hands the batch's poses (and their confidences) through
              # one GPU pass before anything reads them; evaluation, the demo and bench.py see untouched poses.  Everything random is one
              # Philox4x32-10 block of (SEED, global step, clip index), purpose 2 beside the audio augmenter's 0 and 1.
              # SEED: integer in [0, 2^64).  MIRROR_PROB in [0, 1]: the share of draws that mirror the skeleton left/right about the neck
              # (PoseTransforms.mirror_table); with MIRROR_PROB > 0 the per-clip code tables have 2 N rows and a mirrored clip i trains row
              # N + i.  SCALE_PCT p in [0, 50]: a per-clip uniform scale, 256 levels in [1 - p / 100, 1 + p / 100].  ROT_DEG r in [0, 45]: a
              # per-clip in-plane rotation about the neck, 256 levels in [-r, +r] degrees.  PER_CLIP True: the step is left out of the draw,
              # so a clip gets the same transformation at every step (a fixed transformation of the data set).
              "POSE_AUGMENT": {"ENABLE": False, "SEED": 0, "MIRROR_PROB": 0.0, "SCALE_PCT": 0.0, "ROT_DEG": 0.0, "PER_CLIP": False}},
    "TEST": {"BATCH_SIZE": 32, "NUM_RESULT_SAMPLE": 8, "SAVE_VIDEO": True, "SAVE_NPZ": True, "MULTIPLE": 1,
             # extensions (per-clip validation metrics, clip_metrics.ClipMetricsAccumulator / csrc/clip_metrics.hip; DESIGN.md section 22;
             # Voice2Pose only).  CLIP_METRICS True = every test_step also commits its clips' records (keypoint-distance, PCK-hit, speed,
             # velocity-error and, with MULTIPLE > 1, pairwise-diversity sums per body part) to a table on the GPU, and validate() / test() add
             # PCK_<alpha>, PCK, PCK_hands, L2_body / L2_face / L2_hands, speed_ratio, speed_ratio_hands, vel_L2, diversity, diversity_hands
             # and clips_nonfinite to their values: over the tables of ALL ranks (one all-gather), the same bits on every rank.  With SAVE_NPZ
             # the master also writes results/epoch<E>-<TAG>-clip_metrics.npz (the table, its column names, the alphas).  False = the loop
             # as it was.  PCK_ALPHAS: one to four thresholds > 0, as fractions of the larger side of the ground truth's bounding box.
             "CLIP_METRICS": False, "PCK_ALPHAS": [0.1, 0.2],
             # extensions (speech-gesture synchrony, sync_metrics.SyncAccumulator / csrc/sync_metrics.hip; Voice2Pose only;
             # needs DATASET.AUDIO_SR 16000 and DATASET.FPS 15).  SYNC_METRICS True = every test_step also detects the audio onsets of its
             # clips and the motion beats of the final poses (prediction and ground truth, per body part) on the GPU and commits how they line
             # up to a table, and validate() / test() add sync_precision, sync_recall, sync_offset_ms, beat_align, beats_per_s (each also
             # _gt = what the real motion achieves on the same audio, and _hands), onsets_per_s and sync_clips_nonfinite to their values: over
             # the tables of ALL ranks, the same bits on every rank.  With SAVE_NPZ the master also writes
             # results/epoch<E>-<TAG>-sync_metrics.npz.  With DEMO.LONG_FORM the long demo reports the same counts over the whole recording.
             # SYNC_TOLERANCE: a beat within this many seconds of an onset is a hit (floor(300 tol + 0.5) ticks of 1/300 s, 1 .. 150).
             # SYNC_SIGMA: the width in seconds of the Gaussian that beat_align weighs a beat's distance with.  False = the loop as it was.
             "SYNC_METRICS": False, "SYNC_TOLERANCE": 0.1, "SYNC_SIGMA": 0.1,
             # extensions (motion histograms, motion_dist.MotionDistAccumulator / csrc/motion_dist.hip; Voice2Pose only).
             # MOTION_DIST True = every test_step also commits, per clip, the 32-bin histograms of speed, acceleration and jerk magnitudes
             # of the prediction and the ground truth per body part to a table on the GPU, and validate() / test() add hellinger_speed /
             # _accel / _jerk (each also _hands, and _floor = the same distance between two halves of the ground truth), accel_ratio,
             # jerk_ratio (each also _hands) and motion_clips_nonfinite to their values: over the tables of ALL ranks, the same bits on every
             # rank.  With SAVE_NPZ the master also writes results/epoch<E>-<TAG>-motion_metrics.npz (the table, the edges, the merged
             # histograms); with SYS.TENSORBOARD the merged histograms as <val|test>/motion/<speed|accel|jerk>_<pred|gt>_<part>.  False = the
             # loop as it was.  MOTION_DIST_EDGES: None = 2 ** ((j - 15) / 3), j = 0 .. 30, final-pose pixels per frame^o for every order
             # (untuned), else three lists (speed, accel, jerk) of 31 ascending numbers > 0.
             "MOTION_DIST": False, "MOTION_DIST_EDGES": None,
             # extension (oracle-code validation, code_fit.CodeFitter / csrc/code_fit.hip; Voice2Pose with a code table
             # only; needs MULTIPLE 1 and neither CLIP_CODE.SAMPLE_FROM_NORMAL nor TEST_WITH_GT_CODE).  ENABLE True = after its usual forward
             # pass (whose numbers stay as they are) every test_step holds the generator fixed and fits, per clip, the code that explains the
             # clip best -- STEPS Adam iterations at learning rate LR on the clip's own L1 loss, the best iterate kept -- and validate() /
             # test() add L2_dist_fit, lip_sync_error_n_fit, G_reg_loss_fit, fit_loss_first, fit_code_z, fit_clips_nonfinite (and
             # G_reg_loss_table with INIT 'table'; the TEST.CLIP_METRICS values again with the suffix _fit) to their values.  The audio
             # encoder runs once per batch; an iteration is the Conv1d stage forward and backward, the head, and two kernels of code_fit.hip.
             # INIT: the start code -- 'zero', 'mean' (the mean row of the trained table) or 'table' (per clip the best of the mean and
             # CANDIDATES rows floor(j N / M) of the table, one forward pass each).  PRIOR L >= 0 adds L * mean_d((c - mu)^2 / var) / 2
             # with the table's per-dimension mean and unbiased variance.  STEPS (1 .. 1000) and LR (> 0) are UNTUNED defaults: nobody has
             # yet looked for the pair that converges fastest on a trained model.  CANDIDATES 0 .. 64.  False = the loop as it was, no
             # kernel of the fit is launched.
             "FIT_CODE": {"ENABLE": False, "STEPS": 100, "LR": 0.05, "INIT": "mean", "CANDIDATES": 0, "PRIOR": 0.0},
             # extension (precision / recall / density / coverage of the generated gestures, prdc.FeatureSetAccumulator / csrc/prdc.hip;
             # DESIGN.md section 33; Voice2Pose with VOICE2POSE.POSE_ENCODER.NAME only; MULTIPLE 1 .. 16).  ENABLE True = every test_step
             # also commits its clips' pose-encoder features (mu ++ logvar of the ground truth and of every MULTIPLE copy of the prediction)
             # to a table on the GPU, and validate() / test() compare the SET of generated clips with the SET of real clips in the feature
             # space of the FGD: precision (the share of generated rows inside the k-nearest-neighbour ball of some real row: are the
             # gestures plausible?), recall (the share of real rows inside the ball of some generated row: are all templates covered?),
             # density and coverage (their outlier-robust forms).  Sixteen values: precision_mu, recall_mu, density_mu, coverage_mu on the
             # mu columns, the same four with _mu_logvar on all columns, and each of the eight again with _floor = the same metric between
             # the real clips at even and at odd positions of the index-ordered list (what two halves of the real data score at this set
             # size; NaN when a half has at most K rows); prdc_clips_nonfinite counts the clips left out for a NaN / inf feature.  Over the
             # tables of ALL ranks (one all-gather), the same bits on every rank.  With SAVE_NPZ the master also writes
             # results/epoch<E>-<TAG>-prdc.npz (per-row radii, ball counts, nearest real clip, flags, clip indices).  False = the loop as it
             # was, nothing constructed or launched.  K: neighbours of a radius, an integer 1 .. 16; 5 is the value of the density /
             # coverage paper and UNTUNED for validation sets of a few hundred clips.  Not verified: real data, a trained encoder, a
             # multi-GPU run.
             "PRDC": {"ENABLE": False, "K": 5},
             # extension (bootstrap intervals of the clip metrics, bootstrap.clip_metric_intervals / csrc/bootstrap.hip; DESIGN.md section
             # 34; needs CLIP_METRICS).  ENABLE True = validate() / test() resample the clips of the gathered clip-metrics table with
             # replacement REPLICATES times on the GPU (no second all-gather, the same bits on every rank) and add, for every metric key of
             # TEST.CLIP_METRICS, <key>_lo and <key>_hi: the percentile interval of coverage LEVEL, the order statistics at ranks
             # floor(REPLICATES (1 - LEVEL) / 2) from either end of the replicate values.  With FIT_CODE the _fit keys get <key>_fit_lo /
             # _hi too, and one paired run of the fitted against the plain prediction (the same draws for both) adds <key>_fit_gain_lo /
             # _hi, the interval of fitted minus plain, for L2_hands, PCK and PCK_hands.  With SAVE_NPZ the master also writes
             # results/epoch<E>-<TAG>-clip_bootstrap.npz (the replicate values, their names, the point row, n, R, level, seed, part
             # sizes).  The intervals are percentile intervals without bias correction, and they take the clips as independent: clips cut
             # from one recording are not, so on such sets they are optimistic.  FGD, PRDC, synchrony and motion-distance values are not
             # covered.  REPLICATES: an integer 100 .. 20000.  LEVEL in (0, 1).  SEED in [0, 2^64): the Philox key of the draws.  False =
             # the loop as it was, nothing constructed or launched.
             "BOOTSTRAP": {"ENABLE": False, "REPLICATES": 1000, "LEVEL": 0.95, "SEED": 0}},
    "DEMO": {"MULTIPLE": 1, "NUM_SAMPLES": 1, "CODE_INDEX": None, "CODE_INDEX_B": None, "CODE_PATH": None,
             # extensions (the whole-recording demo, long_demo.LongDemo / csrc/long_demo.hip; Voice2Pose only).
             # LONG_FORM True = a demo input of F >= DATASET.NUM_FRAMES frames is generated as overlapping windows of NUM_FRAMES frames (the
             # length the generator was trained at), with one template code for the whole recording, and the windows' final poses are
             # cross-faded into one sequence on the GPU; shorter inputs, and every input with False, take the single pass as it was.  Set
             # DATASET.MAX_DEMO_LENGTH None to get the whole file (with a number the crop happens first).
             # WINDOW_OVERLAP: frames two neighbouring windows share, 0 .. NUM_FRAMES / 2.  LONG_BATCH: windows per forward pass, 1 .. 256.
             # SMOOTH: None, or [m, d] = a Savitzky-Golay filter of half-width m in 1 .. 8 and degree d in 0 .. 2 m over time on the
             # stitched poses.  SEGMENT_FRAMES (>= NUM_FRAMES): videos and long images of a long result are written in pieces of at most
             # this many frames (-part<NN> appended to the file stems when there is more than one).
             "LONG_FORM": False, "WINDOW_OVERLAP": 16, "LONG_BATCH": 32, "SMOOTH": None, "SEGMENT_FRAMES": 900},
    "SYS": {"OUTPUT_DIR": "output/", "CANVAS_SIZE": (720, 1280), "VISUALIZATION_SCALING": 0.85,
            "VIDEO_FORMAT": ["mp4", "img"], "ASYNC_VIDEO_SAVING": False, "LOG_INTERVAL": 100, "NUM_WORKERS": 8,
            "DISTRIBUTED": False, "WORLD_SIZE": 1, "MASTER_ADDR": "localhost", "MASTER_PORT": 21379,
            # extensions of this engine (absent from the reference's configs/default.py:4-97; defaults = the reference's behaviour):
            # STORAGE 'bf16' = BASELINE config 4's arithmetic for the Conv2d chain (ops.set_storage), HIP_GRAPH = replay the train step
            # from a captured hipGraph (graph.GraphedStep, single-GPU runs)
            # CHAIN1D False = the generator's Conv1d blocks one by one: the one-launch chain spins on clusters of co-resident workgroups, so a GPU
            # that two training processes share must not run two of them at once (each would wait for CUs the other one holds until the spin limit
            # trips and the Trainer raises)
            "STORAGE": "f32", "HIP_GRAPH": False, "CHAIN1D": True,
            # RENDER_VIDEO True = TRAIN/TEST.SAVE_VIDEO and the demo write the reference's videos and long images, drawn on the GPU
            # (render.py, video.py; mp4 needs an ffmpeg executable, else the JPEG frames + wav are kept).  False = npz output only.
            "RENDER_VIDEO": False,
            # DEVICE_JPEG True = the video writer takes the JPEG frames of 'mp4' and the long image of 'img' from the GPU encoder (jpeg.py,
            # csrc/jpeg.hip) whenever the pictures are device tensors: only compressed bytes are copied to the host.
            # False = raw frames are copied and PIL encodes them.  VIDEO_FORMAT also takes 'avi' (not in the default list): a Motion-JPEG
            # file with PCM audio that needs no ffmpeg (avi.py); its device frames always go through the GPU encoder.
            "DEVICE_JPEG": False,
            # EPOCH_FIGURES True = at the end of every epoch the master process writes <base>/figures/epoch<E>-clip_code.png, the reference's
            # train/clip_code figure (a 2-component PCA of the clip-code table, scatter-plotted), computed and drawn on the GPU (code_pca.py;
            # DESIGN.md section 12) and logs its explained-variance ratios and axis limits.  False = no figure, the loop as it was.
            "EPOCH_FIGURES": False,
            # DEVICE_FGD True = validate() / test() keep the pose-encoder features on the GPU: every test_step adds its rows to a float64 state of
            # moments (fgd.FGDAccumulator, csrc/fgd.hip) instead of copying them to the host, and FGD_mu / FGD_mu_logvar come from
            # the states of ALL ranks (one all-gather): the value of the whole validation set on every rank, whatever the world size.  False = the
            # reference's loop: host copies per step, scipy sqrtm on the master's shard.
            "DEVICE_FGD": False,
            # TENSORBOARD True = the master process writes a TensorBoard event file into the run's directory (tb_events.py, no tensorboard
            # package needed) with the reference's tags: train/lr_*, train/<loss>, train/epoch_time, train/ETA,
            # train/<figure> (with EPOCH_FIGURES), val/<metric>, test/<metric>, and, with the 'tensorboard' token of VIDEO_FORMAT, the sample
            # videos as animated GIFs that device frames get from the GPU encoder (gif.py, csrc/gif.hip).  False = no event file.
            "TENSORBOARD": False,
            # HISTOGRAM_INTERVAL N (a positive integer; needs TENSORBOARD) = at every train step with global_step % N == 0 the master process
            # adds, for every parameter an optimiser owns, the histograms weights/<name> and grads/<name> (the gradient Adam consumes, before
            # clipping; ema/<name> too with TRAIN.EMA_DECAY), the scalars weight_norm/<name> and grad_norm/<name>, and nonfinite/<name> when a
            # NaN or inf sits in that tensor.  One segmented GPU pass per optimiser buffer (tensor_hist.py, csrc/tensor_hist.hip; DESIGN.md
            # section 20), taken after the step, outside any captured graph.  None = nothing is launched, the loop as it was.
            "HISTOGRAM_INTERVAL": None,
            # CONV_F32_SPLIT (fp32 tensors): Conv2d products as six bf16 MFMA products of an exact three-way bf16 split of both operands, fp32
            # accumulation (csrc/convbf.hip; fp32-grade results, 1.3x faster); False = the fp32-MFMA kernels of rounds 3-4
            "CONV_F32_SPLIT": True,
            # DDP_UNSYNCED_D True = the reference's data-parallel quirk (core/pipelines/voice2pose.py:301,308): DistributedDataParallel
            # all-reduces the gradients of the FIRST backward of a step only, so the discriminator's own backward (the second one of an s2g step)
            # leaves per-rank gradients and the rank's discriminators drift apart.  Default False: this engine synchronises them (dp.GradReducer).
            "DDP_UNSYNCED_D": False,
            # EVAL_WITH_EMA True = validate(), test() and demo() run on the EMA weights (TRAIN.EMA_DECAY, or a checkpoint that carries
            # 'model_ema_state_dict'); the training weights are back, bit for bit, when they return.  False = the training weights.
            "EVAL_WITH_EMA": False,
            # AUDIO_STRIP (the audio under the gestures, audio_strip.py / csrc/audio_strip.hip; Voice2Pose only; needs
            # RENDER_VIDEO, DATASET.AUDIO_SR 16000 and DATASET.FPS 15).  ENABLE True = every pair video, demo video and long image gets a band
            # of HEIGHT rows (a multiple of 16 from 64 to 512) appended below the canvas, drawn on the GPU: the waveform envelope, with MARKS
            # the audio onsets and the motion beats of part 'all' that sync_metrics detects (prediction, and ground truth in pair videos),
            # the mel spectrogram of the clean audio over DB_RANGE dB (20 .. 120) below its largest power and, in videos, a playhead.  A clip
            # of at most SPAN_S seconds (1 .. 60) shows its whole audio; a longer one scrolls with the playhead in the middle.  The skeleton
            # rows of every picture keep their bytes.  False = nothing is imported, constructed or launched; every file as it was.
            "AUDIO_STRIP": {"ENABLE": False, "HEIGHT": 160, "SPAN_S": 4.3, "MARKS": True, "DB_RANGE": 80.0}},
}


class CfgNode(dict):
    def __init__(self, d=None):
        super().__init__()
        object.__setattr__(self, "_frozen", False)
        for k, v in (d or {}).items():
            self[k] = CfgNode(v) if isinstance(v, dict) else v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        if self._frozen:
            raise AttributeError("Attempted to set %s on a frozen CfgNode" % k)
        self[k] = v

    def freeze(self, flag=True):
        object.__setattr__(self, "_frozen", flag)
        for v in self.values():
            if isinstance(v, CfgNode):
                v.freeze(flag)

    def defrost(self):
        self.freeze(False)

    def clone(self):
        return copy.deepcopy(self)

    def _merge(self, other, path=""):
        for k, v in other.items():
            if k not in self:
                raise KeyError("Non-existent config key: %s%s" % (path, k))
            if isinstance(v, dict):
                self[k]._merge(v, path + k + ".")
            else:
                if isinstance(self[k], float) and isinstance(v, (str, int)) and not isinstance(v, bool):
                    v = float(v)  # YAML 1.1 reads "1e-4" as a string
                self[k] = v

    def merge_from_file(self, path):
        with open(path) as f:
            self._merge(yaml.safe_load(f) or {})

    def merge_from_list(self, opts):
        assert len(opts) % 2 == 0, "override list must be KEY VAL pairs"
        for key, val in zip(opts[0::2], opts[1::2]):
            node = self
            parts = key.split(".")
            for p in parts[:-1]:
                node = node[p]
            if parts[-1] not in node:
                raise KeyError("Non-existent config key: %s" % key)
            if isinstance(val, str):
                try:
                    val = ast.literal_eval(val)
                except (ValueError, SyntaxError):
                    pass
            node[parts[-1]] = val


def check_optim_guard(cfg, checkpoint_has_ema=False):
    """Validate the optimiser-safeguard keys; ``checkpoint_has_ema``: the checkpoint being loaded carries 'model_ema_state_dict'."""
    clip, decay = cfg.TRAIN.GRAD_CLIP_NORM, cfg.TRAIN.EMA_DECAY
    if clip is not None and (isinstance(clip, bool) or not isinstance(clip, (int, float)) or not clip > 0):
        raise ValueError("TRAIN.GRAD_CLIP_NORM must be None or a positive number, got %r" % (clip,))
    if decay is not None and (isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0 < decay < 1):
        raise ValueError("TRAIN.EMA_DECAY must be None or a number in (0, 1), got %r" % (decay,))
    if cfg.SYS.EVAL_WITH_EMA and decay is None and not checkpoint_has_ema:
        raise ValueError("SYS.EVAL_WITH_EMA needs an EMA to evaluate: set TRAIN.EMA_DECAY, or load a checkpoint that carries "
                         "'model_ema_state_dict' (one written by a run with TRAIN.EMA_DECAY)")


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and v == v and abs(v) != float('inf')


def check_reg_loss(cfg):
    """Validate VOICE2POSE.GENERATOR.LAMBDA_VEL / REG_MIN_CONFIDENCE / REG_PART_WEIGHTS.  Returns None when all three are at their defaults
    (the plain L1 mean), else (lambda_vel, min_confidence or None, (body, face, hands) or None) as Python floats."""
    g = cfg.VOICE2POSE.GENERATOR
    vel, conf, parts = g.LAMBDA_VEL, g.REG_MIN_CONFIDENCE, g.REG_PART_WEIGHTS
    pre = "VOICE2POSE.GENERATOR."
    if not _is_number(vel) or vel < 0:
        raise ValueError(pre + "LAMBDA_VEL must be a number >= 0, got %r" % (vel,))
    if conf is not None and not _is_number(conf):
        raise ValueError(pre + "REG_MIN_CONFIDENCE must be None or a number, got %r" % (conf,))
    if parts is not None:
        if not isinstance(parts, (list, tuple)) or len(parts) != 3:
            raise ValueError(pre + "REG_PART_WEIGHTS must be None or three numbers [body, face, hands], got %r" % (parts,))
        if not all(_is_number(w) and w >= 0 for w in parts):
            raise ValueError(pre + "REG_PART_WEIGHTS: every weight must be a number >= 0, got %r" % (parts,))
    if vel == 0 and conf is None and parts is None:
        return None
    return float(vel), None if conf is None else float(conf), None if parts is None else tuple(float(w) for w in parts)


def check_bone_loss(cfg):
    """Validate VOICE2POSE.GENERATOR.LAMBDA_BONE / LAMBDA_BONE_DIR / BONE_MIN_LENGTH (and the two keys of ``check_reg_loss`` the limb losses
    reuse).  Returns None when both lambdas are 0 (no limb loss: the step as it was), else
    (lambda_bone, lambda_bone_dir, min_length, min_confidence or None, (body, face, hands) or None) as Python floats."""
    g = cfg.VOICE2POSE.GENERATOR
    bone, bdir, lmin = g.LAMBDA_BONE, g.LAMBDA_BONE_DIR, g.BONE_MIN_LENGTH
    pre = "VOICE2POSE.GENERATOR."
    if not _is_number(bone) or bone < 0:
        raise ValueError(pre + "LAMBDA_BONE must be a number >= 0, got %r" % (bone,))
    if not _is_number(bdir) or bdir < 0:
        raise ValueError(pre + "LAMBDA_BONE_DIR must be a number >= 0, got %r" % (bdir,))
    if not _is_number(lmin) or not lmin > 0:
        raise ValueError(pre + "BONE_MIN_LENGTH must be a number > 0, got %r" % (lmin,))
    if bone == 0 and bdir == 0:
        return None
    reg = check_reg_loss(cfg)
    conf, parts = (None, None) if reg is None else reg[1:]
    if cfg.DATASET.NUM_LANDMARKS != 121:
        raise ValueError(pre + "LAMBDA_BONE / LAMBDA_BONE_DIR need the 121-keypoint skeleton, DATASET.NUM_LANDMARKS is %r"
                         % (cfg.DATASET.NUM_LANDMARKS,))
    return float(bone), float(bdir), float(lmin), conf, parts


def check_clip_metrics(cfg):
    """Validate TEST.CLIP_METRICS / TEST.PCK_ALPHAS.  Returns None with the key off, else the alphas as a tuple of Python floats."""
    on, alphas = cfg.TEST.CLIP_METRICS, cfg.TEST.PCK_ALPHAS
    if not isinstance(on, bool):
        raise ValueError("TEST.CLIP_METRICS must be True or False, got %r" % (on,))
    if not isinstance(alphas, (list, tuple)) or not 1 <= len(alphas) <= 4:
        raise ValueError("TEST.PCK_ALPHAS must be a list of one to four numbers, got %r" % (alphas,))
    if not all(_is_number(a) and a > 0 for a in alphas):
        raise ValueError("TEST.PCK_ALPHAS: every alpha must be a finite number > 0, got %r" % (alphas,))
    if not on:
        return None
    _check_clip_table_key(cfg, "TEST.CLIP_METRICS", "PCK, part errors, speed and diversity of predicted gestures",
                          " (the pairwise diversity of the copies)")
    return tuple(float(a) for a in alphas)


def _check_clip_table_key(cfg, key, what, why_multiple=""):
    """what every per-clip validation table asks of the run: the Voice2Pose pipeline, and TEST.MULTIPLE from 1 to 16"""
    if cfg.PIPELINE_TYPE != "Voice2Pose":
        raise ValueError("%s is a Voice2Pose key (%s), got PIPELINE_TYPE %r" % (key, what, cfg.PIPELINE_TYPE))
    m = cfg.TEST.MULTIPLE
    if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= 16:
        raise ValueError("%s takes TEST.MULTIPLE from 1 to 16%s, got %r" % (key, why_multiple, m))


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def check_fit_code(cfg):
    """Validate TEST.FIT_CODE (ValueError names the key; the ranges are checked whether or not the key is on).  Returns None with ENABLE off,
    else {'steps', 'lr', 'init', 'candidates', 'prior'} as Python values (code_fit.CodeFitter's opts)."""
    f, pre = cfg.TEST.FIT_CODE, "TEST.FIT_CODE."
    on, steps, lr, init, cands, prior = f.ENABLE, f.STEPS, f.LR, f.INIT, f.CANDIDATES, f.PRIOR
    if not isinstance(on, bool):
        raise ValueError(pre + "ENABLE must be True or False, got %r" % (on,))
    if not _is_int(steps) or not 1 <= steps <= 1000:
        raise ValueError(pre + "STEPS must be an integer from 1 to 1000, got %r" % (steps,))
    if not _is_number(lr) or not lr > 0:
        raise ValueError(pre + "LR must be a finite number > 0, got %r" % (lr,))
    if init not in ("zero", "mean", "table"):
        raise ValueError(pre + "INIT must be 'zero', 'mean' or 'table', got %r" % (init,))
    if not _is_int(cands) or not 0 <= cands <= 64:
        raise ValueError(pre + "CANDIDATES must be an integer from 0 to 64, got %r" % (cands,))
    if init == "table" and cands < 1:
        raise ValueError(pre + "CANDIDATES must be at least 1 with INIT 'table' (the table rows to try), got %r" % (cands,))
    if not _is_number(prior) or not prior >= 0:
        raise ValueError(pre + "PRIOR must be a finite number >= 0, got %r" % (prior,))
    if not on:
        return None
    if cfg.PIPELINE_TYPE != "Voice2Pose":
        raise ValueError(pre + "ENABLE is a Voice2Pose key (fitting a template code to a clip), got PIPELINE_TYPE %r" % (cfg.PIPELINE_TYPE,))
    code = cfg.VOICE2POSE.GENERATOR.CLIP_CODE
    if code.DIMENSION is None:
        raise ValueError(pre + "ENABLE needs VOICE2POSE.GENERATOR.CLIP_CODE.DIMENSION: this generator takes no code")
    if not _is_int(code.DIMENSION) or not 1 <= code.DIMENSION <= 256:
        raise ValueError(pre + "ENABLE takes VOICE2POSE.GENERATOR.CLIP_CODE.DIMENSION from 1 to 256, got %r" % (code.DIMENSION,))
    if cfg.VOICE2POSE.GENERATOR.NORM != "IN":
        raise ValueError(pre + "ENABLE needs VOICE2POSE.GENERATOR.NORM 'IN' (an eval-mode BatchNorm stage has no backward pass in this "
                         "engine), got %r" % (cfg.VOICE2POSE.GENERATOR.NORM,))
    m = cfg.TEST.MULTIPLE
    if isinstance(m, bool) or m != 1:
        raise ValueError(pre + "ENABLE needs TEST.MULTIPLE 1 (one fit per clip), got %r" % (m,))
    if code.SAMPLE_FROM_NORMAL:
        raise ValueError(pre + "ENABLE does not go with VOICE2POSE.GENERATOR.CLIP_CODE.SAMPLE_FROM_NORMAL (the fit starts from the table)")
    if code.TEST_WITH_GT_CODE:
        raise ValueError(pre + "ENABLE does not go with VOICE2POSE.GENERATOR.CLIP_CODE.TEST_WITH_GT_CODE (the pose encoder supplies the codes)")
    return {'steps': int(steps), 'lr': float(lr), 'init': init, 'candidates': int(cands), 'prior': float(prior)}


def check_sync_metrics(cfg):
    """Validate TEST.SYNC_METRICS / SYNC_TOLERANCE / SYNC_SIGMA (ValueError names the key).  Returns None with the key off, else
    {'tol_ticks', 'sigma'}."""
    on, tol, sigma = cfg.TEST.SYNC_METRICS, cfg.TEST.SYNC_TOLERANCE, cfg.TEST.SYNC_SIGMA
    if not isinstance(on, bool):
        raise ValueError("TEST.SYNC_METRICS must be True or False, got %r" % (on,))
    if not _is_number(tol):
        raise ValueError("TEST.SYNC_TOLERANCE must be a finite number of seconds, got %r" % (tol,))
    ticks = int(math.floor(300 * float(tol) + 0.5))
    if not 1 <= ticks <= 150:
        raise ValueError("TEST.SYNC_TOLERANCE of %r s is %d ticks of 1/300 s, outside 1 .. 150 (0.5 s)" % (tol, ticks))
    if not _is_number(sigma) or not sigma > 0:
        raise ValueError("TEST.SYNC_SIGMA must be a finite number of seconds > 0, got %r" % (sigma,))
    if not on:
        return None
    _check_clip_table_key(cfg, "TEST.SYNC_METRICS", "audio onsets against the beats of predicted gestures")
    if cfg.DATASET.AUDIO_SR != 16000:
        raise ValueError("TEST.SYNC_METRICS needs DATASET.AUDIO_SR 16000 (an audio hop of 160 samples is 3 ticks of 1/300 s), got %r"
                         % (cfg.DATASET.AUDIO_SR,))
    if cfg.DATASET.FPS != 15:
        raise ValueError("TEST.SYNC_METRICS needs DATASET.FPS 15 (a pose frame is 20 ticks of 1/300 s), got %r" % (cfg.DATASET.FPS,))
    return {'tol_ticks': ticks, 'sigma': float(sigma)}


def check_motion_dist(cfg):
    """Validate TEST.MOTION_DIST / TEST.MOTION_DIST_EDGES (ValueError names the key; the edges are checked whether or not the key is on).
    Returns None with the key off, else {'edges': None for the default ladder, or three tuples of 31 Python floats}."""
    on, edges = cfg.TEST.MOTION_DIST, cfg.TEST.MOTION_DIST_EDGES
    if not isinstance(on, bool):
        raise ValueError("TEST.MOTION_DIST must be True or False, got %r" % (on,))
    if edges is not None:
        if not isinstance(edges, (list, tuple)) or len(edges) != 3 or not all(isinstance(r, (list, tuple)) and len(r) == 31 for r in edges):
            raise ValueError("TEST.MOTION_DIST_EDGES must be None or three lists (speed, accel, jerk) of 31 numbers, got %r" % (edges,))
        for row in edges:
            if not all(_is_number(e) and e > 0 and _is_number(float(e) * float(e)) and float(e) * float(e) > 0 for e in row):
                raise ValueError("TEST.MOTION_DIST_EDGES: every edge must be a finite number > 0 (and so must its square), got %r" % (row,))
            if not all(a < b for a, b in zip(row[:-1], row[1:])):
                raise ValueError("TEST.MOTION_DIST_EDGES: the edges of every order must be strictly ascending, got %r" % (row,))
        edges = tuple(tuple(float(e) for e in row) for row in edges)
    if not on:
        return None
    _check_clip_table_key(cfg, "TEST.MOTION_DIST", "motion histograms of predicted gestures against the ground truth")
    return {'edges': edges}


def check_prdc(cfg):
    """Validate TEST.PRDC (ValueError names the key; K is checked whether or not the key is on).  Returns None with ENABLE off, else
    {'k'} as a Python value (prdc.FeatureSetAccumulator's k)."""
    on, k = cfg.TEST.PRDC.ENABLE, cfg.TEST.PRDC.K
    if not isinstance(on, bool):
        raise ValueError("TEST.PRDC.ENABLE must be True or False, got %r" % (on,))
    if not _is_int(k) or not 1 <= k <= 16:
        raise ValueError("TEST.PRDC.K must be an integer from 1 to 16, got %r" % (k,))
    if not on:
        return None
    _check_clip_table_key(cfg, "TEST.PRDC.ENABLE", "precision / recall / density / coverage of the generated gestures' pose-encoder features")
    if cfg.VOICE2POSE.POSE_ENCODER.NAME is None:
        raise ValueError("TEST.PRDC.ENABLE needs VOICE2POSE.POSE_ENCODER.NAME (the features are the pose encoder's mu and logvar), got None")
    return {'k': int(k)}


def check_bootstrap(cfg):
    """Validate TEST.BOOTSTRAP (ValueError names the key; the ranges are checked whether or not the key is on).  Returns None with ENABLE
    off, else {'replicates', 'level', 'seed', 'rank'} as Python values (rank = floor(REPLICATES (1 - LEVEL) / 2))."""
    from .bootstrap import MAX_REPLICATES, MIN_REPLICATES, rank_of
    b, pre = cfg.TEST.BOOTSTRAP, "TEST.BOOTSTRAP."
    on, reps, level, seed = b.ENABLE, b.REPLICATES, b.LEVEL, b.SEED
    if not isinstance(on, bool):
        raise ValueError(pre + "ENABLE must be True or False, got %r" % (on,))
    if not _is_int(reps) or not MIN_REPLICATES <= reps <= MAX_REPLICATES:
        raise ValueError(pre + "REPLICATES must be an integer from %d to %d, got %r" % (MIN_REPLICATES, MAX_REPLICATES, reps))
    if not _is_number(level) or not 0 < level < 1:
        raise ValueError(pre + "LEVEL must be a number in (0, 1), got %r" % (level,))
    rank = rank_of(reps, level)
    if not 2 * rank < reps:
        raise ValueError(pre + "LEVEL %r puts the rank %d outside [0, REPLICATES / 2)" % (level, rank))
    if not _is_int(seed) or not 0 <= seed < 1 << 64:
        raise ValueError(pre + "SEED must be an integer in [0, 2^64), got %r" % (seed,))
    if not on:
        return None
    if cfg.TEST.CLIP_METRICS is not True:
        raise ValueError(pre + "ENABLE needs TEST.CLIP_METRICS (the intervals are those of the clip-metrics table), got %r"
                         % (cfg.TEST.CLIP_METRICS,))
    return {'replicates': int(reps), 'level': float(level), 'seed': int(seed), 'rank': rank}


def check_augment(cfg):
    """Validate TRAIN.AUGMENT (ValueError names the key).  With ENABLE off the other keys are checked for their type only and None is
    returned; otherwise their ranges too, and {'seed', 'gain_db', 'snr': None or (lo, hi), 'noise_prob', 'shift_ms', 'shift': the largest
    shift in samples, 'polarity', 'freq_masks': (n, w), 'time_masks': (n, w)} comes back as Python values."""
    a, pre = cfg.TRAIN.AUGMENT, "TRAIN.AUGMENT."
    on, seed, gain, snr, prob, shift, pol = a.ENABLE, a.SEED, a.GAIN_DB, a.NOISE_SNR_DB, a.NOISE_PROB, a.SHIFT_MS, a.POLARITY
    if not isinstance(on, bool):
        raise ValueError(pre + "ENABLE must be True or False, got %r" % (on,))
    if not _is_int(seed):
        raise ValueError(pre + "SEED must be an integer, got %r" % (seed,))
    if not _is_number(gain):
        raise ValueError(pre + "GAIN_DB must be a finite number, got %r" % (gain,))
    if snr is not None and (not isinstance(snr, (list, tuple)) or len(snr) != 2 or not all(_is_number(v) for v in snr)):
        raise ValueError(pre + "NOISE_SNR_DB must be None or two finite numbers [lo, hi], got %r" % (snr,))
    if not _is_number(prob):
        raise ValueError(pre + "NOISE_PROB must be a finite number, got %r" % (prob,))
    if not _is_number(shift):
        raise ValueError(pre + "SHIFT_MS must be a finite number, got %r" % (shift,))
    if not isinstance(pol, bool):
        raise ValueError(pre + "POLARITY must be True or False, got %r" % (pol,))
    masks = {}
    for key, widest in (("MEL_FREQ_MASKS", 40), ("MEL_TIME_MASKS", 100)):
        v = a[key]
        if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(_is_int(x) for x in v):
            raise ValueError(pre + key + " must be two integers [n, w], got %r" % (v,))
        masks[key] = (int(v[0]), int(v[1]), widest)
    if not on:
        return None
    if cfg.PIPELINE_TYPE != "Voice2Pose":
        raise ValueError(pre + "ENABLE is a Voice2Pose key (the audio of a train step is augmented before the mel front end), got "
                         "PIPELINE_TYPE %r" % (cfg.PIPELINE_TYPE,))
    if not 0 <= seed < 1 << 64:
        raise ValueError(pre + "SEED must lie in [0, 2^64), got %r" % (seed,))
    if not 0 <= gain <= 40:
        raise ValueError(pre + "GAIN_DB must lie in [0, 40], got %r" % (gain,))
    if snr is not None and not -20 <= snr[0] <= snr[1] <= 80:
        raise ValueError(pre + "NOISE_SNR_DB [lo, hi] needs -20 <= lo <= hi <= 80, got %r" % (snr,))
    if not 0 <= prob <= 1:
        raise ValueError(pre + "NOISE_PROB must lie in [0, 1], got %r" % (prob,))
    if not 0 <= shift <= 500:
        raise ValueError(pre + "SHIFT_MS must lie in [0, 500], got %r" % (shift,))
    for key, (n, w, widest) in masks.items():
        if not 0 <= n <= 4 or not 0 <= w <= widest:
            raise ValueError(pre + key + " [n, w] needs n from 0 to 4 and w from 0 to %d, got %r" % (widest, [n, w]))
    sr = cfg.DATASET.AUDIO_SR
    if not _is_int(sr) or not 1 <= sr <= 1 << 20:
        raise ValueError(pre + "SHIFT_MS needs DATASET.AUDIO_SR as an integer from 1 to 2^20, got %r" % (sr,))
    samples = int(math.floor(float(shift) * sr / 1000.0))
    noisy = snr is not None and prob > 0
    if not (gain > 0 or noisy or samples > 0 or pol or any(n > 0 and w > 0 for n, w, _ in masks.values())):
        raise ValueError(pre + "ENABLE is set while every augmentation sits at its neutral value (GAIN_DB 0, no noise, a shift of 0 samples, "
                         "no POLARITY, no mel masks): set one, or leave ENABLE off")
    return {'seed': int(seed), 'gain_db': float(gain), 'snr': None if snr is None else (float(snr[0]), float(snr[1])), 'noise_prob': float(prob),
            'shift_ms': float(shift), 'shift': samples, 'polarity': pol, 'freq_masks': masks["MEL_FREQ_MASKS"][:2],
            'time_masks': masks["MEL_TIME_MASKS"][:2]}


def check_pose_augment(cfg):
    """Validate TRAIN.POSE_AUGMENT (ValueError names the key).  With ENABLE off the other keys are checked for their type only and None is
    returned; otherwise their ranges too, and {'seed', 'mirror_prob', 'scale_pct', 'rot_deg', 'per_clip'} comes back as Python values."""
    a, pre = cfg.TRAIN.POSE_AUGMENT, "TRAIN.POSE_AUGMENT."
    on, seed, prob, scale, rot, per_clip = a.ENABLE, a.SEED, a.MIRROR_PROB, a.SCALE_PCT, a.ROT_DEG, a.PER_CLIP
    if not isinstance(on, bool):
        raise ValueError(pre + "ENABLE must be True or False, got %r" % (on,))
    if not _is_int(seed):
        raise ValueError(pre + "SEED must be an integer, got %r" % (seed,))
    for key, v in (("MIRROR_PROB", prob), ("SCALE_PCT", scale), ("ROT_DEG", rot)):
        if not _is_number(v):
            raise ValueError(pre + key + " must be a finite number, got %r" % (v,))
    if not isinstance(per_clip, bool):
        raise ValueError(pre + "PER_CLIP must be True or False, got %r" % (per_clip,))
    if not on:
        return None
    if cfg.PIPELINE_TYPE not in ("Voice2Pose", "Pose2Pose"):
        raise ValueError(pre + "ENABLE needs PIPELINE_TYPE Voice2Pose or Pose2Pose, got %r" % (cfg.PIPELINE_TYPE,))
    if not 0 <= seed < 1 << 64:
        raise ValueError(pre + "SEED must lie in [0, 2^64), got %r" % (seed,))
    if not 0 <= prob <= 1:
        raise ValueError(pre + "MIRROR_PROB must lie in [0, 1], got %r" % (prob,))
    if not 0 <= scale <= 50:
        raise ValueError(pre + "SCALE_PCT must lie in [0, 50], got %r" % (scale,))
    if not 0 <= rot <= 45:
        raise ValueError(pre + "ROT_DEG must lie in [0, 45], got %r" % (rot,))
    if cfg.DATASET.NUM_LANDMARKS != 121:
        raise ValueError(pre + "ENABLE needs DATASET.NUM_LANDMARKS 121 (the mirror table and the part roots are those of the 121-keypoint "
                         "skeleton), got %r" % (cfg.DATASET.NUM_LANDMARKS,))
    if not (prob > 0 or scale > 0 or rot > 0):
        raise ValueError(pre + "ENABLE is set while every augmentation sits at its neutral value (MIRROR_PROB 0, SCALE_PCT 0, ROT_DEG 0): "
                         "set one, or leave ENABLE off")
    return {'seed': int(seed), 'mirror_prob': float(prob), 'scale_pct': float(scale), 'rot_deg': float(rot), 'per_clip': per_clip}


def check_long_demo(cfg):
    """Validate DEMO.LONG_FORM / WINDOW_OVERLAP / LONG_BATCH / SMOOTH / SEGMENT_FRAMES (ValueError names the key).  Returns None with the key
    off, else {'overlap', 'batch', 'smooth': None or (m, d), 'segment'}."""
    d, W = cfg.DEMO, cfg.DATASET.NUM_FRAMES
    on, O, batch, smooth, seg = d.LONG_FORM, d.WINDOW_OVERLAP, d.LONG_BATCH, d.SMOOTH, d.SEGMENT_FRAMES
    if not isinstance(on, bool):
        raise ValueError("DEMO.LONG_FORM must be True or False, got %r" % (on,))
    if not _is_int(O) or O < 0:
        raise ValueError("DEMO.WINDOW_OVERLAP must be an integer >= 0, got %r" % (O,))
    if not _is_int(batch) or not 1 <= batch <= 256:
        raise ValueError("DEMO.LONG_BATCH must be an integer from 1 to 256 (windows per forward pass), got %r" % (batch,))
    if smooth is not None:
        if not isinstance(smooth, (list, tuple)) or len(smooth) != 2 or not all(_is_int(v) for v in smooth):
            raise ValueError("DEMO.SMOOTH must be None or two integers [m, d], got %r" % (smooth,))
        if not 1 <= smooth[0] <= 8 or not 0 <= smooth[1] <= 2 * smooth[0]:
            raise ValueError("DEMO.SMOOTH [m, d] needs a half-width m from 1 to 8 and a degree d from 0 to 2 m, got %r" % (smooth,))
    if not _is_int(seg) or seg < 1:
        raise ValueError("DEMO.SEGMENT_FRAMES must be a positive integer, got %r" % (seg,))
    if not on:  # (the bounds that depend on DATASET.NUM_FRAMES hold for a run that uses the keys)
        return None
    if cfg.PIPELINE_TYPE != "Voice2Pose":
        raise ValueError("DEMO.LONG_FORM is a Voice2Pose key (windowed inference from a recording), got PIPELINE_TYPE %r" % (cfg.PIPELINE_TYPE,))
    if not _is_int(W) or W < 2:
        raise ValueError("DEMO.LONG_FORM needs windows of DATASET.NUM_FRAMES >= 2 frames, got %r" % (W,))
    if 2 * O > W:
        raise ValueError("DEMO.WINDOW_OVERLAP must be at most DATASET.NUM_FRAMES / 2 = %d / 2, got %r" % (W, O))
    if seg < W:
        raise ValueError("DEMO.SEGMENT_FRAMES must be at least DATASET.NUM_FRAMES = %d, got %r" % (W, seg))
    if cfg.VOICE2POSE.GENERATOR.CLIP_CODE.TEST_WITH_GT_CODE:
        raise ValueError("DEMO.LONG_FORM cannot run with VOICE2POSE.GENERATOR.CLIP_CODE.TEST_WITH_GT_CODE: a demo input has no ground truth")
    return {'overlap': O, 'batch': batch, 'smooth': None if smooth is None else (smooth[0], smooth[1]), 'segment': seg}


def check_audio_strip(cfg):
    """Validate SYS.AUDIO_STRIP (ValueError names the key; the numbers are checked whether or not the key is on).  Returns None with the key
    off, else {'height', 'span_s', 'marks', 'db_range'}."""
    a, pre = cfg.SYS.AUDIO_STRIP, "SYS.AUDIO_STRIP."
    on, height, span, marks, db = a.ENABLE, a.HEIGHT, a.SPAN_S, a.MARKS, a.DB_RANGE
    if not isinstance(on, bool):
        raise ValueError(pre + "ENABLE must be True or False, got %r" % (on,))
    if not isinstance(marks, bool):
        raise ValueError(pre + "MARKS must be True or False, got %r" % (marks,))
    if not _is_int(height) or height % 16 or not 64 <= height <= 512:
        raise ValueError(pre + "HEIGHT must be a multiple of 16 from 64 to 512 (rows of the band), got %r" % (height,))
    if not _is_number(span) or not 1 <= span <= 60:
        raise ValueError(pre + "SPAN_S must be a number of seconds from 1 to 60, got %r" % (span,))
    if not _is_number(db) or not 20 <= db <= 120:
        raise ValueError(pre + "DB_RANGE must be a number of decibels from 20 to 120, got %r" % (db,))
    if not on:
        return None
    if not cfg.SYS.RENDER_VIDEO:
        raise ValueError(pre + "ENABLE needs SYS.RENDER_VIDEO: the band goes under the rendered pictures")
    if cfg.PIPELINE_TYPE != "Voice2Pose":
        raise ValueError(pre + "ENABLE is a Voice2Pose key (Pose2Pose has no audio), got PIPELINE_TYPE %r" % (cfg.PIPELINE_TYPE,))
    if cfg.DATASET.AUDIO_SR != 16000:
        raise ValueError(pre + "ENABLE needs DATASET.AUDIO_SR 16000 (a mel hop is 160 samples, a tick 160 / 3), got %r" % (cfg.DATASET.AUDIO_SR,))
    if cfg.DATASET.FPS != 15:
        raise ValueError(pre + "ENABLE needs DATASET.FPS 15 (a pose frame is 20 ticks of 1/300 s), got %r" % (cfg.DATASET.FPS,))
    if cfg.SYS.DEVICE_JPEG or "avi" in cfg.SYS.VIDEO_FORMAT:  # the GPU encoder takes pictures of at most 65535 rows and columns (jpeg.py)
        H, W = (int(v) for v in cfg.SYS.CANVAS_SIZE)
        if max(H + height, W) > 65535:
            raise ValueError(pre + "HEIGHT: the GPU JPEG encoder (SYS.DEVICE_JPEG, 'avi') takes at most 65535 rows and columns, got "
                             "%d + %d rows of %d" % (H, height, W))
    return {'height': int(height), 'span_s': float(span), 'marks': marks, 'db_range': float(db)}


def check_histograms(cfg):
    """Validate SYS.HISTOGRAM_INTERVAL: None or a positive integer, and then SYS.TENSORBOARD must be set (there is nowhere else to write)."""
    n = getattr(cfg.SYS, 'HISTOGRAM_INTERVAL', None)
    if n is None:
        return
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError("SYS.HISTOGRAM_INTERVAL must be None or a positive integer, got %r" % (n,))
    if not getattr(cfg.SYS, 'TENSORBOARD', False):
        raise ValueError("SYS.HISTOGRAM_INTERVAL needs SYS.TENSORBOARD: the histograms go to the TensorBoard event file")


def get_cfg_defaults():
    return CfgNode(_DEFAULTS)


def load_cfg(config_file=None, opts=()):
    """main.py:29-33 -- defaults <- yaml <- KEY VAL list, frozen."""
    cfg = get_cfg_defaults()
    if config_file:
        cfg.merge_from_file(config_file)
    cfg.merge_from_list(list(opts))
    cfg.freeze()
    return cfg
