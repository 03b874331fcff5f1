"""ctypes binding of libwk.so (include/wk_api.h) -- the MI355X batched walker engine.

This is plumbing for tests and bench.py: every call goes straight to the C ABI and
from there to HIP kernels on gfx950.  There is no CPU fallback: if libwk.so is
missing or no GPU is visible, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# WK_LIB selects an alternative in-tree build (kernel A/B experiments)
LIB_PATH = os.environ.get("WK_LIB") or os.path.join(os.path.dirname(_HERE), "libwk.so")

STATE_FLOATS = 112
NPARAM = 6149
NPARAM_CRITIC = 897
NPAIRS = 9
NEV = 16  # WK_NEV event counters (wk_count_events)
IPC_HANDLE_BYTES = 128  # WK_IPC_HANDLE_BYTES: IPC handle + the device's PCI bus id
EVENTS = ["joint", "aabb_ll", "aabb_lf", "aabb_bf", "sat_ll", "sat_lf", "sat_bf", "imp_ll",
          "imp_lf", "imp_bf", "contacts", "substeps", "env_steps", "resets", "steps_lf", "steps_satll"]
ST_TORQUE, ST_POS, ST_PREV, ST_STEPS, ST_POSTRESET, ST_TERMINAL, ST_EPISODES = (
    100, 104, 106, 108, 109, 110, 111)
MATERIALS = {"Carpet": 0, "Ice": 1, "Rubber": 2, "Metal": 3, "Wood": 4, "Paper": 5,
             "Titanium": 6, "SuperRubber": 7}

# every symbol include/wk_api.h declares (checked by tests/test_boundary.py)
EXPORTS = [
    "wk_config_defaults", "wk_version", "wk_create", "wk_destroy", "wk_last_error", "wk_sync",
    "wk_num_envs", "wk_reset", "wk_set_materials", "wk_set_offsets", "wk_step",
    "wk_step_device", "wk_step_sampled", "wk_step_traced", "wk_get_obs", "wk_get_state", "wk_set_state",
    "wk_get_body_view", "wk_set_scene", "wk_get_prop_view", "wk_get_weights", "wk_set_weights", "wk_get_adam", "wk_set_adam",
    "wk_policy_sample", "wk_value", "wk_rollout", "wk_rollout_stats_get", "wk_get_trajectory",
    "wk_set_trajectory", "wk_compute_returns", "wk_ppo_update", "wk_train_batch",
    "wk_minibatch_gradient", "wk_save_weights", "wk_load_weights", "wk_format_weights",
    "wk_parse_weights", "wk_checkpoint_save", "wk_checkpoint_load",
    "wk_host_settings_defaults", "wk_config_to_json", "wk_config_from_json",
    "wk_config_save_json", "wk_config_load_json", "wk_collect_data", "wk_episode_log_count",
    "wk_episode_log_drain", "wk_loss_log_drain", "wk_write_data_file",
    "wk_comm_unique_id", "wk_comm_init", "wk_comm_init_host", "wk_allreduce_test", "wk_profile_enable",
    "wk_profile_get", "wk_profile_reset", "wk_count_events", "wk_snapshot", "wk_time_gradient",
    "wk_time_gradient_ex", "wk_grad_kernel", "wk_rollout_mapping",
    "wk_comm_ipc_handle", "wk_comm_init_ipc", "wk_comm_info", "wk_comm_set_timeout",
    "wk_comm_xch_profile", "wk_comm_xch_stamps", "wk_check_state", "wk_take_actions",
    "wk_object_update", "wk_joint_step", "wk_body_order",
    "wk_net_param_count", "wk_num_params", "wk_format_weights_net", "wk_parse_weights_net",
    "wk_get_bootstrap_values", "wk_set_bootstrap_values",
    "wk_policy_stats", "wk_update_stats_get", "wk_evaluate", "wk_evaluate_time",
    "wk_grad_norms_get", "wk_set_learning_rate", "wk_get_learning_rate",
    "wk_get_log_std", "wk_set_log_std", "wk_set_log_std_adam", "wk_log_std_gradient",
    "wk_reward_norm_defaults", "wk_reward_norm_config", "wk_reward_norm_get", "wk_reward_norm_set",
    "wk_reward_norm_get_acc", "wk_reward_norm_set_acc", "wk_reward_norm_update", "wk_get_scaled_rewards",
    "wk_render_defaults", "wk_render", "wk_render_device", "wk_render_states",
    "wk_comm_records", "wk_ppo_sums_add", "wk_ppo_stats_from_sums", "wk_log_std_grad_from_sums",
    "wk_policy_sums", "wk_policy_stats_global",
]
COMM_RECORD_WORDS = 16  # WK_COMM_RECORD_WORDS: one record of the record exchange, 64-bit words
RECORD_STATS, RECORD_REWARD_NORM = 1, 2  # the kinds in a record's header word


def check_state(state):
    """wk_check_state (host only, no device): (ok, first bad walker, first bad record body)"""
    import numpy as np
    st = np.ascontiguousarray(state, dtype=np.float32)
    be, bb = C.c_int(), C.c_int()
    lib = load_library()
    r = lib.wk_check_state(st.ctypes.data, int(st.size // STATE_FLOATS), C.byref(be), C.byref(bb))
    return r == 0, be.value, bb.value


class WkConfig(C.Structure):
    """wk_config up to MaxGradNorm (its first 128 bytes): Hyperparameters.cs:80-121 names and
    defaults + batched extensions.  The library reads and writes the whole wk_config, which is
    WkConfigLogStd below: that is what default_config() returns and every call takes."""
    _fields_ = [
        ("GameSpeed", C.c_int), ("Iterations", C.c_int), ("MaxTimesteps", C.c_int),
        ("RoughFloor", C.c_int), ("Epochs", C.c_int), ("BatchSize", C.c_int),
        ("UseGAE", C.c_int), ("NormalizeAdvantages", C.c_int), ("Gamma", C.c_float),
        ("Lambda", C.c_float), ("Epsilon", C.c_float), ("LogStandardDeviation", C.c_float),
        ("Alpha", C.c_float), ("Beta1", C.c_float), ("Beta2", C.c_float),
        ("AdamEpsilon", C.c_float), ("CriticNeuralNetwork", C.c_char_p),
        ("ActorNeuralNetwork", C.c_char_p), ("DeltaTime", C.c_float), ("Horizon", C.c_int),
        ("Minibatch", C.c_int), ("MinibatchGlobal", C.c_int), ("EnvOffset", C.c_int),
        ("RandomizeStart", C.c_int), ("RandomizeMaterial", C.c_int),
        ("LanesPerWalker", C.c_int), ("NetworkKernels", C.c_int),
        ("ReturnsMode", C.c_int), ("TargetKL", C.c_float), ("MaxGradNorm", C.c_float),
    ]


class WkConfigLogStd(WkConfig):
    """wk_config as include/wk_api.h declares it: WkConfig's fields, then the five of the trained
    log-std appended (a ctypes subclass lays its fields out after the base's; the base ends on an
    8-byte boundary, so the offsets are the C struct's)."""
    _fields_ = [
        ("LearnLogStd", C.c_int), ("LogStdAlpha", C.c_float), ("EntropyCoef", C.c_float),
        ("LogStdMin", C.c_float), ("LogStdMax", C.c_float),
    ]


assert C.sizeof(WkConfig) == WkConfigLogStd.LearnLogStd.offset == 128 and C.sizeof(WkConfigLogStd) == 152


class HostSettings(C.Structure):
    """wk_host_settings: SerializableHyperparameters' host-only fields (Hyperparameters.cs:11-77)."""
    _fields_ = [
        ("CollectData", C.c_int), ("SaveWeights", C.c_int),
        ("CriticNeuralNetwork", C.c_char * 256), ("ActorNeuralNetwork", C.c_char * 256),
        ("CriticWeightFileName", C.c_char * 256), ("ActorWeightFileName", C.c_char * 256),
        ("FilePath", C.c_char * 1024),
    ]


class EpisodeRec(C.Structure):
    _fields_ = [("total_reward", C.c_float), ("env", C.c_int32), ("length", C.c_int32),
                ("step", C.c_uint32)]


EPISODE_DTYPE = np.dtype([("total_reward", np.float32), ("env", np.int32), ("length", np.int32),
                          ("step", np.uint32)])


class PairTrace(C.Structure):
    _fields_ = [("aabb_hit", C.c_uint8 * 9), ("sat_hit", C.c_uint8 * 9),
                ("n_contacts", C.c_uint8 * 9), ("pad", C.c_uint8 * 5),
                ("normal", (C.c_float * 2) * 9), ("depth", C.c_float * 9),
                ("contact", ((C.c_float * 2) * 2) * 9), ("impulse", (C.c_float * 2) * 9),
                ("joint_depth", C.c_float * 4), ("joint_impulse", C.c_float * 4)]


TRACE_DTYPE = np.dtype([("aabb_hit", np.uint8, 9), ("sat_hit", np.uint8, 9),
                        ("n_contacts", np.uint8, 9), ("pad", np.uint8, 5),
                        ("normal", np.float32, (9, 2)), ("depth", np.float32, 9),
                        ("contact", np.float32, (9, 2, 2)), ("impulse", np.float32, (9, 2)),
                        ("joint_depth", np.float32, 4), ("joint_impulse", np.float32, 4)])
assert TRACE_DTYPE.itemsize == C.sizeof(PairTrace) == 140 + 144 + 72 + 32


class BodyView(C.Structure):
    _fields_ = [("n_vertices", C.c_int), ("vertices", (C.c_float * 2) * 6),
                ("centroid", C.c_float * 2), ("linear_velocity", C.c_float * 2),
                ("angular_velocity", C.c_float), ("angle", C.c_float), ("collided", C.c_int),
                ("is_static", C.c_int)]


SHAPES = {"Square": 0, "Triangle": 1, "Hexagon": 2}
MAX_PROPS, PROP_MAXV, SCENE_MAX_VERTS = 4, 24, 32


class Prop(C.Structure):
    """wk_prop: <Shape>.FromSize + SmoothCorners + velocities + acceleration (include/wk_api.h)"""
    _fields_ = [("shape", C.c_int32), ("smooth", C.c_int32), ("material", C.c_int32),
                ("is_static", C.c_int32), ("cx", C.c_float), ("cy", C.c_float),
                ("size", C.c_float), ("vx", C.c_float), ("vy", C.c_float), ("w", C.c_float),
                ("ax", C.c_float), ("ay", C.c_float)]


def make_prop(shape="Square", smooth=0, material="Wood", is_static=False, cx=0.0, cy=0.0,
              size=40.0, vx=0.0, vy=0.0, w=0.0, ax=0.0, ay=0.0):
    return Prop(SHAPES.get(shape, shape), int(smooth), MATERIALS.get(material, material),
                int(bool(is_static)), cx, cy, size, vx, vy, w, ax, ay)


class PropView(C.Structure):
    _fields_ = [("n_vertices", C.c_int), ("vertices", (C.c_float * 2) * PROP_MAXV),
                ("centroid", C.c_float * 2), ("linear_velocity", C.c_float * 2),
                ("angular_velocity", C.c_float), ("angle", C.c_float), ("is_static", C.c_int)]

    def vertex_array(self):
        return np.array(self.vertices, np.float32)[:self.n_vertices]


class PpoArgs(C.Structure):
    _fields_ = [("epochs", C.c_int), ("minibatch", C.c_int), ("minibatch_global", C.c_int),
                ("update_index", C.c_uint32)]


class RolloutStats(C.Structure):
    _fields_ = [("reward_sum", C.c_double), ("episodes", C.c_int64), ("env_steps", C.c_int64),
                ("fault_or", C.c_uint32), ("pad", C.c_int32)]


class PpoStats(C.Structure):
    """wk_ppo_stats: the current policy on the trajectory buffer (wk_policy_stats) / the last
    per-epoch check of a TargetKL > 0 update (wk_update_stats_get)"""
    _fields_ = [("samples", C.c_int64), ("skipped", C.c_int64), ("kl", C.c_double),
                ("kl_k1", C.c_double), ("clip_fraction", C.c_double), ("ratio_max", C.c_double),
                ("surrogate", C.c_double), ("value_loss", C.c_double),
                ("explained_variance", C.c_double), ("epochs_run", C.c_int32),
                ("stopped_early", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PpoSums(C.Structure):
    """wk_ppo_sums: the raw sums the statistics passes end in (wk_policy_sums), as the record
    exchange gathers them and the host divides them"""
    _fields_ = [("rows", C.c_int64), ("skipped", C.c_int64), ("clipped", C.c_int64),
                ("kl", C.c_double), ("k1", C.c_double), ("surr", C.c_double), ("sr", C.c_double),
                ("srr", C.c_double), ("se", C.c_double), ("see", C.c_double), ("rmax", C.c_double),
                ("term", C.c_double), ("zz", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


PPO_SUMS = PpoSums


def _sums(s):
    """a PpoSums from a PpoSums or its dict"""
    return s if isinstance(s, PpoSums) else PpoSums(**{k: s[k] for k, _ in PpoSums._fields_})


def sums_add(acc, x):
    """wk_ppo_sums_add: acc + x as a new dict (integers and doubles add, rmax is the larger, a NaN
    stays) -- the fold step of the record exchange, so the order of a chain of calls matters"""
    a = PpoSums.from_buffer_copy(_sums(acc))
    load_library().wk_ppo_sums_add(C.byref(a), C.byref(_sums(x)))
    return a.as_dict()


def stats_from_sums(s):
    """wk_ppo_stats_from_sums: the statistics' dict (policy_stats' keys) from the raw sums"""
    st = PpoStats()
    load_library().wk_ppo_stats_from_sums(C.byref(_sums(s)), C.byref(st))
    return st.as_dict()


def log_std_grad_from_sums(s, entropy_coef=0.0):
    """wk_log_std_grad_from_sums: the log-std gradient's dict (log_std_gradient's keys)"""
    g = LogStdGrad()
    load_library().wk_log_std_grad_from_sums(C.byref(_sums(s)), float(entropy_coef), C.byref(g))
    return g.as_dict()


class GradNorms(C.Structure):
    """wk_grad_norms: the gradient norms of a MaxGradNorm > 0 context's Adam steps since the last
    ppo_update / train_batch / minibatch_gradient began (index 0 the critic, 1 the actor)"""
    _fields_ = [("steps", C.c_int64), ("clipped", C.c_int64 * 2), ("nonfinite", C.c_int64 * 2),
                ("norm_last", C.c_double * 2), ("norm_max", C.c_double * 2),
                ("norm_sum", C.c_double * 2), ("scale_last", C.c_float * 2), ("pad", C.c_int32 * 2)]

    def as_dict(self):
        return {k: (getattr(self, k) if k == "steps" else tuple(getattr(self, k)))
                for k, _ in self._fields_ if k != "pad"}


class LogStdGrad(C.Structure):
    """wk_log_std_grad: the clipped surrogate's derivative by the scalar log-std over the
    trajectory buffer (wk_log_std_gradient), host-divided"""
    _fields_ = [("samples", C.c_int64), ("skipped", C.c_int64), ("grad_surrogate", C.c_double),
                ("grad", C.c_double), ("z2_mean", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LogStdState(C.Structure):
    """wk_log_std_state: the policy's log-std and the state of its Adam step (wk_get_log_std)"""
    _fields_ = [("log_std", C.c_float), ("std", C.c_float), ("t", C.c_int32), ("pad", C.c_int32),
                ("m", C.c_double), ("v", C.c_double), ("entropy", C.c_double),
                ("grad_last", C.c_double), ("steps", C.c_int64), ("clamped", C.c_int64),
                ("nonfinite", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class RewardNormArgs(C.Structure):
    """wk_reward_norm_args: the switch and the two constants of the reward normalisation"""
    _fields_ = [("enable", C.c_int32), ("frozen", C.c_int32), ("clip", C.c_float), ("epsilon", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RewardNorm(C.Structure):
    """wk_reward_norm: the running statistics of the walkers' discounted returns, the scale the
    last pass used and that pass's counters (wk_reward_norm_get)"""
    _fields_ = [("count", C.c_int64), ("mean", C.c_double), ("m2", C.c_double), ("var", C.c_double),
                ("scale", C.c_float), ("clip", C.c_float), ("epsilon", C.c_float),
                ("enabled", C.c_int32), ("frozen", C.c_int32), ("pad", C.c_int32),
                ("rows", C.c_int64), ("clipped", C.c_int64), ("nonfinite", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


EVAL_MAX_EPISODES = 16  # WK_EVAL_MAX_EPISODES
EVAL_FELL, EVAL_TIME_LIMIT, EVAL_SUCCESS, EVAL_UNFINISHED = 0, 1, 2, 3  # enum wk_eval_end
EVAL_STARTS = {"reset": 0, "create": 1}  # wk_eval_args.start
# the evaluation fold's grid (csrc/wk_kernels.h): at most EVAL_FOLD_MAX_BLOCKS blocks of
# EVAL_FOLD_BLOCK lanes, one lane per walker, striding over the walkers
EVAL_FOLD_BLOCK, EVAL_FOLD_MAX_BLOCKS = 256, 64


class EvalArgs(C.Structure):
    _fields_ = [("episodes", C.c_int32), ("stochastic", C.c_int32), ("start", C.c_int32),
                ("max_steps", C.c_int32), ("poll", C.c_int32), ("rng_step0", C.c_uint32)]


class EvalRec(C.Structure):
    _fields_ = [("total_reward", C.c_float), ("length", C.c_int32), ("distance", C.c_float),
                ("final_x", C.c_float), ("end", C.c_int32), ("env", C.c_int32)]


EVAL_DTYPE = np.dtype([("total_reward", np.float32), ("length", np.int32), ("distance", np.float32),
                       ("final_x", np.float32), ("end", np.int32), ("env", np.int32)])
assert EVAL_DTYPE.itemsize == C.sizeof(EvalRec) == 24


class EvalStats(C.Structure):
    """wk_eval_stats: the fold of an evaluation's finished episodes (wk_evaluate)"""
    _fields_ = [("episodes", C.c_int64), ("unfinished", C.c_int64), ("fell", C.c_int64),
                ("timed_out", C.c_int64), ("succeeded", C.c_int64), ("env_steps", C.c_int64),
                ("reward_mean", C.c_double), ("reward_std", C.c_double),
                ("reward_min", C.c_double), ("reward_max", C.c_double),
                ("length_mean", C.c_double), ("length_min", C.c_int32), ("length_max", C.c_int32),
                ("distance_mean", C.c_double), ("distance_max", C.c_double),
                ("fault_or", C.c_uint32), ("steps_run", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


RENDER_MAX_VIEWS, RENDER_MAX_DIM, RENDER_MAX_SEGMENTS = 4096, 2048, 160  # WK_RENDER_MAX_*
# the renderer's tile (csrc/wk_render.h): one block of 256 threads per 64 x 16 pixels of one view
RENDER_TILE_W, RENDER_TILE_H = 64, 16


class RenderArgs(C.Structure):
    """wk_render_args: the frame, the window (scale, origin, follow) and what to draw"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("scale", C.c_float), ("ox", C.c_float),
                ("oy", C.c_float), ("follow", C.c_int32), ("line_px", C.c_float), ("marker_x", C.c_float),
                ("joints", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


def render_args(**args):
    """wk_render_defaults (550 x 325 at scale 0.5 from (-50, 400), no follow, line_px 1, no marker,
    joints on) with the given fields replaced"""
    a = RenderArgs()
    load_library().wk_render_defaults(C.byref(a))
    for k, v in args.items():
        if k == "pad" or k not in dict(RenderArgs._fields_):
            raise KeyError(f"unknown wk_render_args field {k}")
        setattr(a, k, v)
    return a


# the statistics kernels' grids (csrc/wk_kernels.h): the built-in kernel runs at most
# STATS_MAX_BLOCKS blocks of STATS_WAVES waves, each wave striding over the 16-row chunks; the
# general kernel at most NET_MAX_BLOCKS one-wave blocks of equally many consecutive 16-row tiles
STATS_MAX_BLOCKS, STATS_WAVES, NET_MAX_BLOCKS, STATS_ROWS = 512, 4, 1024, 16


class Profile(C.Structure):
    _fields_ = [("physics_ms", C.c_double), ("physics_launches", C.c_int64),
                ("physics_env_steps", C.c_int64), ("grad_ms", C.c_double),
                ("grad_launches", C.c_int64), ("reduce_ms", C.c_double),
                ("reduce_launches", C.c_int64), ("adam_ms", C.c_double),
                ("adam_launches", C.c_int64), ("allreduce_ms", C.c_double),
                ("allreduce_calls", C.c_int64), ("returns_ms", C.c_double),
                ("returns_launches", C.c_int64), ("update_ms", C.c_double),
                ("update_calls", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None
# wk_host_allreduce_fn: int (*)(float* buf, int n, void* user)
HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p)
# wk_host_allgather_fn: int (const uint64_t* mine, uint64_t* all, void* user)
HOST_ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p)


def load_library(path=None):
    """Load libwk.so (raises OSError if it was not built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise OSError(f"libwk.so not built at {p}: run __graft_entry__.build() "
                      "(or make -C ppo-bipedalwalker_amd)")
    # PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64 / librccl with the same
    # SONAMEs as /opt/rocm.  Loading torch first makes libwk.so bind to those copies, so
    # one process has exactly one HIP runtime (torch.cuda.synchronize() then also covers
    # libwk's stream).  Loading libwk first would pull in a second runtime under torch.
    try:
        import torch  # noqa: F401
    except Exception:  # torch is plumbing only; libwk.so stands alone without it
        pass
    lib = C.CDLL(p)
    P, I, F, U32, U64 = C.c_void_p, C.c_int, C.c_float, C.c_uint32, C.c_uint64
    fp = C.POINTER(C.c_float)
    sig = {
        "wk_config_defaults": (None, [C.POINTER(WkConfigLogStd)]),
        "wk_version": (C.c_char_p, []),
        "wk_create": (I, [C.POINTER(WkConfigLogStd), I, I, U64, C.POINTER(P)]),
        "wk_destroy": (I, [P]),
        "wk_last_error": (C.c_char_p, [P]),
        "wk_sync": (I, [P]),
        "wk_num_envs": (I, [P]),
        "wk_reset": (I, [P, P]),
        "wk_set_materials": (I, [P, P]),
        "wk_set_offsets": (I, [P, P]),
        "wk_step": (I, [P, P, I, P, P, P, P]),
        "wk_step_device": (I, [P, P, I, P, P, P, P]),
        "wk_step_traced": (I, [P, P, P]),
        "wk_step_sampled": (I, [P, I, P, P, P, P, P, P, P, P, P]),
        "wk_get_obs": (I, [P, P]),
        "wk_get_state": (I, [P, P]),
        "wk_set_state": (I, [P, P]),
        "wk_get_body_view": (I, [P, I, I, C.POINTER(BodyView)]),
        "wk_set_scene": (I, [P, P, I]),
        "wk_get_prop_view": (I, [P, I, I, C.POINTER(PropView)]),
        "wk_get_weights": (I, [P, P]),
        "wk_set_weights": (I, [P, P]),
        "wk_get_adam": (I, [P, P, P, C.POINTER(C.c_int)]),
        "wk_set_adam": (I, [P, P, P, I]),
        "wk_policy_sample": (I, [P, I, P, P, P, P, P, P]),
        "wk_value": (I, [P, I, P, P]),
        "wk_rollout": (I, [P, I]),
        "wk_rollout_stats_get": (I, [P, C.POINTER(RolloutStats)]),
        "wk_get_trajectory": (I, [P, P, P, P, P, P, P, P, P]),
        "wk_set_trajectory": (I, [P, I, P, P, P, P, P, P]),
        "wk_compute_returns": (I, [P]),
        "wk_ppo_update": (I, [P, C.POINTER(PpoArgs), fp, fp]),
        "wk_train_batch": (I, [P, I, F, P, P, P, P, P, fp, fp, P, I, C.POINTER(C.c_int)]),
        "wk_minibatch_gradient": (I, [P, I, F, P, P, P, P, P, fp, fp, P, C.POINTER(C.c_int)]),
        "wk_save_weights": (I, [P, C.c_char_p, C.c_char_p]),
        "wk_load_weights": (I, [P, C.c_char_p, C.c_char_p]),
        "wk_format_weights": (I, [P, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]),
        "wk_parse_weights": (I, [C.c_char_p, C.c_char_p, P]),
        "wk_checkpoint_save": (I, [P, C.c_char_p]),
        "wk_checkpoint_load": (I, [P, C.c_char_p]),
        "wk_host_settings_defaults": (None, [C.POINTER(HostSettings)]),
        "wk_config_to_json": (I, [C.POINTER(WkConfigLogStd), C.POINTER(HostSettings), C.c_char_p, C.c_size_t]),
        "wk_config_from_json": (I, [C.c_char_p, C.POINTER(WkConfigLogStd), C.POINTER(HostSettings)]),
        "wk_config_save_json": (I, [C.c_char_p, C.POINTER(WkConfigLogStd), C.POINTER(HostSettings)]),
        "wk_config_load_json": (I, [C.c_char_p, C.POINTER(WkConfigLogStd), C.POINTER(HostSettings)]),
        "wk_collect_data": (I, [P, I]),
        "wk_episode_log_count": (I, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "wk_episode_log_drain": (I, [P, P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "wk_loss_log_drain": (I, [P, P, P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "wk_write_data_file": (I, [C.c_char_p, P, C.c_int64, P, C.c_int64, P, C.c_int64]),
        "wk_comm_unique_id": (I, [P]),
        "wk_comm_init": (I, [P, I, I, P]),
        "wk_allreduce_test": (I, [P, P, I]),
        "wk_comm_init_host": (I, [P, I, I, HOST_ALLREDUCE_FN, P]),
        "wk_time_gradient": (I, [P, I, I, C.POINTER(C.c_double)]),
        "wk_time_gradient_ex": (I, [P, I, I, I, C.POINTER(C.c_double)]),
        "wk_rollout_mapping": (I, [P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int64)]),
        "wk_comm_info": (I, [P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "wk_grad_kernel": (I, [P, I]),
        "wk_comm_ipc_handle": (I, [P, P]),
        "wk_comm_init_ipc": (I, [P, I, I, P]),
        "wk_comm_set_timeout": (I, [P, C.c_double]),
        "wk_comm_xch_profile": (I, [P, I]),
        "wk_check_state": (I, [P, I, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "wk_take_actions": (I, [P, I, P]),
        "wk_object_update": (I, [P, I, C.c_float]),
        "wk_joint_step": (I, [P]),
        "wk_body_order": (I, [P, I, P, C.POINTER(C.c_int)]),
        "wk_comm_xch_stamps": (I, [P, P, I, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "wk_profile_enable": (I, [P, I]),
        "wk_profile_get": (I, [P, C.POINTER(Profile)]),
        "wk_profile_reset": (I, [P]),
        "wk_count_events": (I, [P, I, P]),
        "wk_snapshot": (I, [P, I]),
        "wk_net_param_count": (I, [C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "wk_num_params": (I, [P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "wk_format_weights_net": (I, [C.c_char_p, C.c_char_p, P, C.c_char_p, C.c_size_t, C.c_char_p,
                                      C.c_size_t]),
        "wk_parse_weights_net": (I, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, P]),
        "wk_get_bootstrap_values": (I, [P, P]),
        "wk_set_bootstrap_values": (I, [P, P]),
        "wk_policy_stats": (I, [P, C.POINTER(PpoStats), P, P]),
        "wk_update_stats_get": (I, [P, C.POINTER(PpoStats)]),
        "wk_evaluate": (I, [P, C.POINTER(EvalArgs), C.POINTER(EvalStats), P]),
        "wk_evaluate_time": (I, [P, I, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "wk_grad_norms_get": (I, [P, C.POINTER(GradNorms)]),
        "wk_set_learning_rate": (I, [P, F]),
        "wk_get_learning_rate": (I, [P, fp]),
        "wk_get_log_std": (I, [P, C.POINTER(LogStdState)]),
        "wk_set_log_std": (I, [P, F]),
        "wk_set_log_std_adam": (I, [P, C.c_double, C.c_double, I]),
        "wk_log_std_gradient": (I, [P, C.POINTER(LogStdGrad)]),
        "wk_reward_norm_defaults": (None, [C.POINTER(RewardNormArgs)]),
        "wk_reward_norm_config": (I, [P, C.POINTER(RewardNormArgs)]),
        "wk_reward_norm_get": (I, [P, C.POINTER(RewardNorm)]),
        "wk_reward_norm_set": (I, [P, C.c_int64, C.c_double, C.c_double]),
        "wk_reward_norm_get_acc": (I, [P, P]),
        "wk_reward_norm_set_acc": (I, [P, P]),
        "wk_reward_norm_update": (I, [P]),
        "wk_get_scaled_rewards": (I, [P, P]),
        "wk_render_defaults": (None, [C.POINTER(RenderArgs)]),
        "wk_render": (I, [P, C.POINTER(RenderArgs), P, I, P]),
        "wk_render_device": (I, [P, C.POINTER(RenderArgs), P, I, P]),
        "wk_render_states": (I, [P, C.POINTER(RenderArgs), P, P, I, P]),
        "wk_comm_records": (I, [P, P, P]),
        "wk_ppo_sums_add": (None, [C.POINTER(PpoSums), C.POINTER(PpoSums)]),
        "wk_ppo_stats_from_sums": (None, [C.POINTER(PpoSums), C.POINTER(PpoStats)]),
        "wk_log_std_grad_from_sums": (None, [C.POINTER(PpoSums), F, C.POINTER(LogStdGrad)]),
        "wk_policy_sums": (I, [P, C.POINTER(PpoSums), C.POINTER(PpoSums)]),
        "wk_policy_stats_global": (I, [P, C.POINTER(PpoStats)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    _ = U32
    if path is None:
        _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        a = a.reshape(shape)
    return a


WK_ERR_COMM = -4  # enum wk_status (include/wk_api.h)


class WkError(RuntimeError):
    pass


def default_config(**overrides):
    lib = load_library()
    c = WkConfigLogStd()  # (the whole wk_config; a bare WkConfig would be 24 bytes short)
    lib.wk_config_defaults(C.byref(c))
    for k, v in overrides.items():
        if not hasattr(c, k):
            raise KeyError(f"unknown wk_config field {k}")
        if isinstance(v, str):
            v = v.encode()
        setattr(c, k, v)
    return c


def default_host_settings():
    h = HostSettings()
    load_library().wk_host_settings_defaults(C.byref(h))
    return h


def config_to_json(cfg=None, host=None):
    """Hyperparameters.SerializeJson (Hyperparameters.cs:124-131): the indented JSON text."""
    lib = load_library()
    cp = None if cfg is None else C.byref(cfg)
    hp = None if host is None else C.byref(host)
    need = -lib.wk_config_to_json(cp, hp, None, 0)
    if need <= 0:
        raise WkError(f"wk_config_to_json: {lib.wk_last_error(None).decode()}")
    buf = C.create_string_buffer(need)
    rc = lib.wk_config_to_json(cp, hp, buf, need)
    if rc != 0:
        raise WkError(f"wk_config_to_json failed ({rc}): {lib.wk_last_error(None).decode()}")
    return buf.value.decode()


def config_from_json(text, cfg=None, host=None):
    """Hyperparameters.DeserializeJson (Hyperparameters.cs:135-187) applied to (cfg, host)
    (defaults when None).  Returns (cfg, host, corrections): corrections lists the
    ValidateVariables messages (values reset to defaults).  Raises WkError when the
    document is malformed or a value is out of range (nothing is changed then)."""
    lib = load_library()
    cfg = default_config() if cfg is None else cfg
    host = default_host_settings() if host is None else host
    raw = text.encode() if isinstance(text, str) else bytes(text)
    rc = lib.wk_config_from_json(raw, C.byref(cfg), C.byref(host))
    msg = lib.wk_last_error(None).decode()
    if rc < 0:
        raise WkError(f"wk_config_from_json failed ({rc}): {msg}")
    cfg._host = host  # cfg's network strings point into host's buffers
    return cfg, host, (msg.split("\n") if rc > 0 else [])


def write_data_file(path, total_rewards, critic_losses, actor_losses):
    """ConsoleRenderer.CreateDataFile (ConsoleRenderer.cs:124-135)."""
    lib = load_library()
    r, c, a = (np.ascontiguousarray(x, np.float32) for x in (total_rewards, critic_losses, actor_losses))
    rc = lib.wk_write_data_file(os.fsencode(path), _ptr(r), r.size, _ptr(c), c.size, _ptr(a), a.size)
    if rc != 0:
        raise WkError(f"wk_write_data_file failed ({rc}): {lib.wk_last_error(None).decode()}")


def _net(s):
    return None if s is None else (s if isinstance(s, bytes) else s.encode())


def net_param_count(critic=None, actor=None):
    """wk_net_param_count: (critic, actor) parameter counts of two network strings (None: the
    default string); WkError for an invalid string or one beyond the general kernels' limits."""
    lib = load_library()
    nc, na = C.c_int(), C.c_int()
    rc = lib.wk_net_param_count(_net(critic), _net(actor), C.byref(nc), C.byref(na))
    if rc != 0:
        raise WkError(f"wk_net_param_count failed ({rc}): {lib.wk_last_error(None).decode()}")
    return nc.value, na.value


def format_weights(params, critic=None, actor=None):
    """(critic_text, actor_text) of a parameter vector in the reference's weights-file format
    (NeuralNetwork.Save NeuralNetwork.cs:159-176; one line per entry, newline-terminated);
    critic / actor: the network strings (None: the default ones, a WK_NPARAM vector)."""
    lib = load_library()
    p = _f32(params, (sum(net_param_count(critic, actor)),))
    cn, an = _net(critic), _net(actor)
    need = -lib.wk_format_weights_net(cn, an, _ptr(p), None, 0, None, 0)
    if need <= 0:
        raise WkError("wk_format_weights_net: size query failed")
    cb, ab = C.create_string_buffer(need), C.create_string_buffer(need)
    rc = lib.wk_format_weights_net(cn, an, _ptr(p), cb, need, ab, need)
    if rc != 0:
        raise WkError(f"wk_format_weights_net failed ({rc})")
    return cb.value.decode(), ab.value.decode()


def parse_weights(critic_text, actor_text, critic=None, actor=None):
    """parameter vector from weights-file texts (NeuralNetwork.Load NeuralNetwork.cs:94-115) of
    the networks critic / actor (None: the default strings, WK_NPARAM values)."""
    lib = load_library()
    p = np.empty(sum(net_param_count(critic, actor)), np.float32)
    rc = lib.wk_parse_weights_net(_net(critic), _net(actor), critic_text.encode(), actor_text.encode(),
                                  _ptr(p))
    if rc != 0:
        raise WkError(f"wk_parse_weights failed ({rc}): {lib.wk_last_error(None).decode()}")
    return p


class Engine:
    """One wk_ctx: n_env walkers on one GPU."""

    def __init__(self, n_env, seed=20250905, device=0, **cfg):
        self.lib = load_library()
        self.cfg = default_config(**cfg)
        self.n = int(n_env)
        self.seed = int(seed)
        h = C.c_void_p()
        rc = self.lib.wk_create(C.byref(self.cfg), int(device), self.n, self.seed, C.byref(h))
        if rc != 0:
            raise WkError(f"wk_create failed ({rc}): {self.lib.wk_last_error(None).decode()}")
        self.h = h
        nc, na = C.c_int(), C.c_int()
        self._chk(self.lib.wk_num_params(self.h, C.byref(nc), C.byref(na)), "wk_num_params")
        self.nparam_critic, self.nparam = nc.value, nc.value + na.value
        self._t_valid = 0  # rows of the trajectory buffer (scaled_rewards)

    # -- plumbing --
    def _chk(self, rc, what):
        if rc != 0:
            msg = f"{what} failed ({rc}): {self.lib.wk_last_error(self.h).decode()}"
            if rc == WK_ERR_COMM and getattr(self, "_host_ar_error", None):
                msg += f" [host all-reduce callback raised {self._host_ar_error}; fatal for the job]"
                self._host_ar_error = None
            if rc == WK_ERR_COMM and getattr(self, "_rx_error", None):
                msg += f" [record all-gather callback raised {self._rx_error}; fatal for the job]"
                self._rx_error = None
            raise WkError(msg)

    def close(self):
        if getattr(self, "h", None):
            self.lib.wk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        self._chk(self.lib.wk_sync(self.h), "wk_sync")

    # -- environment --
    def reset(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self._chk(self.lib.wk_reset(self.h, _ptr(m)), "wk_reset")

    def set_materials(self, mat):
        m = np.ascontiguousarray(mat, dtype=np.int32)
        self._chk(self.lib.wk_set_materials(self.h, _ptr(m)), "wk_set_materials")

    def set_offsets(self, dx):
        d = _f32(dx)
        self._chk(self.lib.wk_set_offsets(self.h, _ptr(d)), "wk_set_offsets")

    def step(self, actions=None, k=1):
        """k env-steps; actions [k, n, 4] (unclipped) or None to sample from the policy."""
        a = None if actions is None else _f32(actions, (k, self.n, 4))
        obs = np.empty((k, self.n, 12), np.float32)
        rew = np.empty((k, self.n), np.float32)
        done = np.empty((k, self.n), np.uint8)
        fault = np.empty(self.n, np.uint32)
        self._chk(self.lib.wk_step(self.h, _ptr(a), int(k), _ptr(obs), _ptr(rew), _ptr(done),
                                   _ptr(fault)), "wk_step")
        return obs, rew, done, fault

    def step_sampled(self, k=1):
        """Environment.Update with the agent's sampling (wk_step_sampled): the Trajectory
        entries of Environment.cs:70-89 -- states before each step, unclipped actions,
        per-dimension log-probabilities, values, rewards, dones -- the next states, and the
        torso position after each step before any auto-reset (Environment.cs:113-119)."""
        n = self.n
        out = dict(states=np.empty((k, n, 12), np.float32), actions=np.empty((k, n, 4), np.float32),
                   logp=np.empty((k, n, 4), np.float32), values=np.empty((k, n), np.float32),
                   rewards=np.empty((k, n), np.float32), dones=np.empty((k, n), np.uint8),
                   next_obs=np.empty((k, n, 12), np.float32), fault=np.empty(n, np.uint32),
                   position=np.empty((k, n, 2), np.float32))
        self._chk(self.lib.wk_step_sampled(
            self.h, int(k), _ptr(out["states"]), _ptr(out["actions"]), _ptr(out["logp"]),
            _ptr(out["values"]), _ptr(out["rewards"]), _ptr(out["dones"]), _ptr(out["next_obs"]),
            _ptr(out["fault"]), _ptr(out["position"])), "wk_step_sampled")
        return out

    def step_device(self, d_actions, k, d_obs, d_rew, d_done, d_fault):
        """Device-pointer variant (ints or None) on the context's stream; no sync."""
        self._chk(self.lib.wk_step_device(self.h, d_actions, int(k), d_obs, d_rew, d_done,
                                          d_fault), "wk_step_device")

    def step_traced(self, actions):
        a = _f32(actions, (self.n, 4))
        tr = np.zeros((self.n, self.cfg.Iterations), TRACE_DTYPE)
        self._chk(self.lib.wk_step_traced(self.h, _ptr(a), _ptr(tr)), "wk_step_traced")
        return tr

    def get_obs(self):
        o = np.empty((self.n, 12), np.float32)
        self._chk(self.lib.wk_get_obs(self.h, _ptr(o)), "wk_get_obs")
        return o

    def get_state(self):
        s = np.empty((self.n, STATE_FLOATS), np.float32)
        self._chk(self.lib.wk_get_state(self.h, _ptr(s)), "wk_get_state")
        return s

    def set_state(self, s):
        s = _f32(s, (self.n, STATE_FLOATS))
        self._chk(self.lib.wk_set_state(self.h, _ptr(s)), "wk_set_state")

    def body_view(self, env, body):
        v = BodyView()
        self._chk(self.lib.wk_get_body_view(self.h, int(env), int(body), C.byref(v)),
                  "wk_get_body_view")
        return v

    def set_scene(self, props):
        """scene props for every walker (Prop structures / make_prop(...)); [] removes them"""
        arr = (Prop * max(1, len(props)))(*props)
        self._chk(self.lib.wk_set_scene(self.h, C.cast(arr, C.c_void_p), len(props)),
                  "wk_set_scene")

    def prop_view(self, env, k):
        v = PropView()
        self._chk(self.lib.wk_get_prop_view(self.h, int(env), int(k), C.byref(v)),
                  "wk_get_prop_view")
        return v

    # -- policy --
    def get_weights(self):
        p = np.empty(self.nparam, np.float32)
        self._chk(self.lib.wk_get_weights(self.h, _ptr(p)), "wk_get_weights")
        return p

    def set_weights(self, p):
        p = _f32(p, (self.nparam,))
        self._chk(self.lib.wk_set_weights(self.h, _ptr(p)), "wk_set_weights")

    def get_adam(self):
        m = np.empty(self.nparam, np.float32)
        v = np.empty(self.nparam, np.float32)
        t = C.c_int()
        self._chk(self.lib.wk_get_adam(self.h, _ptr(m), _ptr(v), C.byref(t)), "wk_get_adam")
        return m, v, t.value

    def set_adam(self, m, v, t):
        m = _f32(m, (self.nparam,))
        v = _f32(v, (self.nparam,))
        self._chk(self.lib.wk_set_adam(self.h, _ptr(m), _ptr(v), int(t)), "wk_set_adam")

    def save_weights(self, critic_path, actor_path):
        """PPOAgent.Save (PPOAgent.cs:192-213): critic / actor weights text files."""
        self._chk(self.lib.wk_save_weights(self.h, os.fsencode(critic_path), os.fsencode(actor_path)),
                  "wk_save_weights")

    def load_weights(self, critic_path, actor_path):
        """PPOAgent.Load over NeuralNetwork.Load (NeuralNetwork.cs:94-115), strict errors."""
        self._chk(self.lib.wk_load_weights(self.h, os.fsencode(critic_path), os.fsencode(actor_path)),
                  "wk_load_weights")

    def checkpoint_save(self, path):
        """Binary checkpoint: weights, Adam state, walker records and Philox counters."""
        self._chk(self.lib.wk_checkpoint_save(self.h, os.fsencode(path)), "wk_checkpoint_save")

    def checkpoint_load(self, path):
        self._chk(self.lib.wk_checkpoint_load(self.h, os.fsencode(path)), "wk_checkpoint_load")
        self._t_valid = 0  # (loading invalidates the trajectory buffer)

    # -- data collection (ConsoleRenderer.AddTotalEpisodeReward / AddCriticLoss / AddActorLoss) --
    def collect_data(self, on=True):
        self._chk(self.lib.wk_collect_data(self.h, int(bool(on))), "wk_collect_data")

    def episode_log_count(self):
        e, u = C.c_int64(), C.c_int64()
        self._chk(self.lib.wk_episode_log_count(self.h, C.byref(e), C.byref(u)), "wk_episode_log_count")
        return e.value, u.value

    def drain_episodes(self):
        """finished episodes since the last drain (structured array EPISODE_DTYPE) and the
        number dropped by overflow"""
        cnt, _ = self.episode_log_count()
        out = np.empty(cnt, EPISODE_DTYPE)
        n, dropped = C.c_int64(), C.c_int64()
        self._chk(self.lib.wk_episode_log_drain(self.h, _ptr(out) if cnt else None, cnt, C.byref(n),
                                                C.byref(dropped)), "wk_episode_log_drain")
        return out[:n.value], dropped.value

    def drain_losses(self):
        """(critic, actor) diagnostics of each PPO update since the last drain"""
        _, cnt = self.episode_log_count()
        cap = min(cnt, 1 << 16)
        c, a = np.empty(cap, np.float32), np.empty(cap, np.float32)
        n, dropped = C.c_int64(), C.c_int64()
        self._chk(self.lib.wk_loss_log_drain(self.h, _ptr(c) if cap else None, _ptr(a) if cap else None,
                                             cap, C.byref(n), C.byref(dropped)), "wk_loss_log_drain")
        return c[:n.value], a[:n.value]

    def policy_sample(self, obs, env_ids=None, steps=None):
        obs = _f32(obs)
        n = obs.shape[0]
        ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
        st = None if steps is None else np.ascontiguousarray(steps, np.uint32)
        mean = np.empty((n, 4), np.float32)
        act = np.empty((n, 4), np.float32)
        lp = np.empty((n, 4), np.float32)
        self._chk(self.lib.wk_policy_sample(self.h, n, _ptr(obs), _ptr(ids), _ptr(st), _ptr(mean),
                                            _ptr(act), _ptr(lp)), "wk_policy_sample")
        return mean, act, lp

    def value(self, obs):
        obs = _f32(obs)
        v = np.empty(obs.shape[0], np.float32)
        self._chk(self.lib.wk_value(self.h, obs.shape[0], _ptr(obs), _ptr(v)), "wk_value")
        return v

    # -- rollout / PPO --
    def rollout(self, horizon=0):
        self._chk(self.lib.wk_rollout(self.h, int(horizon)), "wk_rollout")
        self._t_valid = int(horizon) if horizon > 0 else int(self.cfg.Horizon)

    def rollout_stats(self):
        s = RolloutStats()
        self._chk(self.lib.wk_rollout_stats_get(self.h, C.byref(s)), "wk_rollout_stats_get")
        return s

    def get_trajectory(self, horizon):
        n = self.n * horizon
        out = dict(states=np.empty((horizon, self.n, 12), np.float32),
                   actions=np.empty((horizon, self.n, 4), np.float32),
                   logp=np.empty((horizon, self.n, 4), np.float32),
                   rewards=np.empty((horizon, self.n), np.float32),
                   dones=np.empty((horizon, self.n), np.uint8),
                   values=np.empty((horizon, self.n), np.float32),
                   returns=np.empty((horizon, self.n), np.float32),
                   advantages=np.empty((horizon, self.n), np.float32))
        assert n == out["rewards"].size
        self._chk(self.lib.wk_get_trajectory(
            self.h, _ptr(out["states"]), _ptr(out["actions"]), _ptr(out["logp"]),
            _ptr(out["rewards"]), _ptr(out["dones"]), _ptr(out["values"]), _ptr(out["returns"]),
            _ptr(out["advantages"])), "wk_get_trajectory")
        return out

    def set_trajectory(self, states, actions, logp, rewards, dones, values):
        T = rewards.shape[0]
        args = [_f32(states), _f32(actions), _f32(logp), _f32(rewards),
                np.ascontiguousarray(dones, np.uint8), _f32(values)]
        self._chk(self.lib.wk_set_trajectory(self.h, int(T), *[_ptr(a) for a in args]),
                  "wk_set_trajectory")
        self._t_valid = int(T)

    def compute_returns(self):
        self._chk(self.lib.wk_compute_returns(self.h), "wk_compute_returns")

    def get_bootstrap_values(self):
        """wk_get_bootstrap_values (ReturnsMode = 1): the value each walker's reverse scan starts
        from -- after a rollout, value(get_obs())"""
        v = np.empty(self.n, np.float32)
        self._chk(self.lib.wk_get_bootstrap_values(self.h, _ptr(v)), "wk_get_bootstrap_values")
        return v

    def set_bootstrap_values(self, v):
        """wk_set_bootstrap_values (ReturnsMode = 1): replace them (zeros for complete episodes);
        the next compute_returns / ppo_update recomputes the returns"""
        v = _f32(v, (self.n,))
        self._chk(self.lib.wk_set_bootstrap_values(self.h, _ptr(v)), "wk_set_bootstrap_values")

    def policy_stats(self, per_sample=False):
        """wk_policy_stats: the current actor and critic on every row of the trajectory buffer --
        approximate KL to the collecting policy, clip fraction, largest ratio, surrogate, value
        loss and explained variance as a dict; per_sample=True also returns the rows' fp32
        log-densities [T, n, 4] and values [T, n] (skipped rows included)"""
        st = PpoStats()
        if not per_sample:
            self._chk(self.lib.wk_policy_stats(self.h, C.byref(st), None, None), "wk_policy_stats")
            return st.as_dict()
        # (the buffer's valid horizon is the library's to know: room for the configured one)
        lp = np.zeros((self.cfg.Horizon, self.n, 4), np.float32)
        v = np.zeros((self.cfg.Horizon, self.n), np.float32)
        self._chk(self.lib.wk_policy_stats(self.h, C.byref(st), _ptr(lp), _ptr(v)), "wk_policy_stats")
        T = (st.samples + st.skipped) // self.n
        return st.as_dict(), lp[:T], v[:T]

    def policy_sums(self, global_=False):
        """wk_policy_sums: the raw sums of the log-std pass over this rank's trajectory buffer as a
        dict.  global_=True returns (local, global): on a record-exchange context (comm_records) a
        COLLECTIVE call whose second dict is the ranks' records folded in rank order, the same
        bytes on every rank; on a context with no communicator the local record twice"""
        loc, glo = PpoSums(), PpoSums()
        self._chk(self.lib.wk_policy_sums(self.h, C.byref(loc), C.byref(glo) if global_ else None),
                  "wk_policy_sums")
        return (loc.as_dict(), glo.as_dict()) if global_ else loc.as_dict()

    def policy_stats_global(self):
        """wk_policy_stats_global: policy_stats' dict over all the ranks' shards (collective on a
        record-exchange context; this context's own without a communicator)"""
        st = PpoStats()
        self._chk(self.lib.wk_policy_stats_global(self.h, C.byref(st)), "wk_policy_stats_global")
        return st.as_dict()

    def update_stats(self):
        """wk_update_stats_get: the last per-epoch check of the last ppo_update of a TargetKL > 0
        context (with epochs_run and stopped_early) as a dict"""
        st = PpoStats()
        self._chk(self.lib.wk_update_stats_get(self.h, C.byref(st)), "wk_update_stats_get")
        return st.as_dict()

    def grad_norms(self):
        """wk_grad_norms_get: the per-network gradient norms of the Adam steps of the last
        ppo_update / train_batch of a MaxGradNorm > 0 context as a dict (it synchronises)"""
        g = GradNorms()
        self._chk(self.lib.wk_grad_norms_get(self.h, C.byref(g)), "wk_grad_norms_get")
        return g.as_dict()

    def set_learning_rate(self, alpha):
        """wk_set_learning_rate: Alpha from the next Adam step on (finite, >= 0)"""
        self._chk(self.lib.wk_set_learning_rate(self.h, float(alpha)), "wk_set_learning_rate")

    def get_learning_rate(self):
        a = C.c_float()
        self._chk(self.lib.wk_get_learning_rate(self.h, C.byref(a)), "wk_get_learning_rate")
        return a.value

    def log_std(self):
        """wk_get_log_std: the policy's log-std, std and entropy per dimension, and on a
        LearnLogStd = 1 context the Adam state of the scalar and the last update's counters"""
        s = LogStdState()
        self._chk(self.lib.wk_get_log_std(self.h, C.byref(s)), "wk_get_log_std")
        return s.as_dict()

    def set_log_std(self, s):
        """wk_set_log_std: the log-std every later launch uses (finite, inside (-5, 5), on a
        LearnLogStd = 1 context inside [LogStdMin, LogStdMax]); keeps the scalar's Adam state"""
        self._chk(self.lib.wk_set_log_std(self.h, float(s)), "wk_set_log_std")

    def set_log_std_adam(self, m, v, t):
        """wk_set_log_std_adam (LearnLogStd = 1): the scalar's Adam moments and step count"""
        self._chk(self.lib.wk_set_log_std_adam(self.h, float(m), float(v), int(t)), "wk_set_log_std_adam")

    def log_std_gradient(self):
        """wk_log_std_gradient: the clipped surrogate's derivative by the log-std over the
        trajectory buffer at the current weights and log-std, as a dict (it synchronises and
        changes nothing)"""
        g = LogStdGrad()
        self._chk(self.lib.wk_log_std_gradient(self.h, C.byref(g)), "wk_log_std_gradient")
        return g.as_dict()

    def reward_norm(self, enable=True, clip=10.0, epsilon=1e-8, frozen=False):
        """wk_reward_norm_config: scale the rewards the returns kernels read by the running std of
        the walkers' discounted returns (clamped to +-clip; epsilon is added to the variance).
        frozen: scale with the statistics as they are.  The raw rewards stay what they are."""
        a = RewardNormArgs(int(enable), int(frozen), float(clip), float(epsilon))
        self._chk(self.lib.wk_reward_norm_config(self.h, C.byref(a)), "wk_reward_norm_config")

    def reward_norm_state(self):
        """wk_reward_norm_get: count, mean, m2, var, scale, the arguments and the last pass's
        counters (zeros and scale 1 on a context never enabled)"""
        s = RewardNorm()
        self._chk(self.lib.wk_reward_norm_get(self.h, C.byref(s)), "wk_reward_norm_get")
        return s.as_dict()

    def set_reward_norm_state(self, count, mean, m2):
        """wk_reward_norm_set: replace the running statistics; the scale follows"""
        self._chk(self.lib.wk_reward_norm_set(self.h, int(count), float(mean), float(m2)), "wk_reward_norm_set")

    def reward_acc(self):
        """wk_reward_norm_get_acc: every walker's running discounted return"""
        a = np.empty(self.n, np.float32)
        self._chk(self.lib.wk_reward_norm_get_acc(self.h, _ptr(a)), "wk_reward_norm_get_acc")
        return a

    def set_reward_acc(self, a):
        a = _f32(a, (self.n,))
        self._chk(self.lib.wk_reward_norm_set_acc(self.h, _ptr(a)), "wk_reward_norm_set_acc")

    def reward_norm_update(self):
        """wk_reward_norm_update: the full pass (scan, merge, apply) on the current trajectory
        buffer -- after set_trajectory, whose data is otherwise scaled but not learned"""
        self._chk(self.lib.wk_reward_norm_update(self.h), "wk_reward_norm_update")

    def scaled_rewards(self, horizon=None):
        """wk_get_scaled_rewards: the [T][n] rewards the returns kernels read, T the rows of the
        last rollout / set_trajectory of this object (or `horizon`)"""
        T = self._t_valid if horizon is None else int(horizon)
        out = np.empty((T, self.n), np.float32)
        self._chk(self.lib.wk_get_scaled_rewards(self.h, _ptr(out)), "wk_get_scaled_rewards")
        return out

    def evaluate(self, episodes=1, stochastic=False, start="reset", max_steps=0, poll=0, rng_step0=0,
                 records=False):
        """wk_evaluate: every walker plays `episodes` complete episodes under the current actor
        (its mean action, or sampled with stochastic=True) on a private copy of the walker state --
        nothing the training run can observe changes.  start: "reset" (as after reset()) or
        "create" (episode-0 body order).  Returns the statistics as a dict; records=True also
        returns the per-episode records, a structured array EVAL_DTYPE [episodes, n]"""
        a = EvalArgs(int(episodes), int(bool(stochastic)), int(EVAL_STARTS.get(start, start)),
                     int(max_steps), int(poll), int(rng_step0))
        st = EvalStats()
        rec = np.zeros((max(1, min(int(episodes), EVAL_MAX_EPISODES)), self.n), EVAL_DTYPE) if records else None
        self._chk(self.lib.wk_evaluate(self.h, C.byref(a), C.byref(st), _ptr(rec)), "wk_evaluate")
        return (st.as_dict(), rec) if records else st.as_dict()

    def evaluate_time(self, reps=64):
        """wk_evaluate_time: mean ms per launch of the evaluation's (accounting kernel, fold) on
        the last evaluate()'s private block"""
        s, f = C.c_double(), C.c_double()
        self._chk(self.lib.wk_evaluate_time(self.h, int(reps), C.byref(s), C.byref(f)), "wk_evaluate_time")
        return s.value, f.value

    @staticmethod
    def _views(envs):
        return np.ascontiguousarray([0] if envs is None else envs, dtype=np.int32).reshape(-1)

    def render(self, envs=None, **args):
        """wk_render: the listed walkers (None: walker 0; repeats allowed) as they are now, drawn on
        the device -- floor, bodies in the material's colour, joint squares by torque, props, an
        optional marker -- as uint8 [n, H, W, 4] RGBA, row 0 at the top.  args: wk_render_args
        fields (width, height, scale, ox, oy, follow, line_px, marker_x, joints)"""
        a, ids = render_args(**args), self._views(envs)
        img = np.empty((ids.size, a.height, a.width, 4), np.uint8)
        self._chk(self.lib.wk_render(self.h, C.byref(a), _ptr(ids), ids.size, _ptr(img)), "wk_render")
        return img

    def render_states(self, states, envs, **args):
        """wk_render_states: host records [n, STATE_FLOATS] (get_state's layout) drawn as if walker
        envs[i] had record states[i]; material, terrain and props are that walker's"""
        a, ids = render_args(**args), self._views(envs)
        st = _f32(states, (ids.size, STATE_FLOATS))
        img = np.empty((ids.size, a.height, a.width, 4), np.uint8)
        self._chk(self.lib.wk_render_states(self.h, C.byref(a), _ptr(st), _ptr(ids), ids.size, _ptr(img)),
                  "wk_render_states")
        return img

    def render_device(self, ptr, envs, **args):
        """wk_render_device: the same frames into device memory at `ptr` (an int, for example a torch
        uint8 tensor's data_ptr(); 4-byte aligned, n * H * W * 4 bytes) on the context's stream; no
        copy and no synchronise.  Returns the image's shape"""
        a, ids = render_args(**args), self._views(envs)
        self._chk(self.lib.wk_render_device(self.h, C.byref(a), _ptr(ids), ids.size, C.c_void_p(int(ptr))),
                  "wk_render_device")
        return (ids.size, a.height, a.width, 4)

    def ppo_update(self, epochs=0, minibatch=0, minibatch_global=0, update_index=0, sync=True):
        """Whole PPO update; returns the last minibatch's (critic, actor) diagnostics, or
        (None, None) with sync=False (then nothing waits on the stream)."""
        a = PpoArgs(int(epochs), int(minibatch), int(minibatch_global), int(update_index))
        if not sync:
            self._chk(self.lib.wk_ppo_update(self.h, C.byref(a), None, None), "wk_ppo_update")
            return None, None
        cd, ad = C.c_float(), C.c_float()
        self._chk(self.lib.wk_ppo_update(self.h, C.byref(a), C.byref(cd), C.byref(ad)),
                  "wk_ppo_update")
        return cd.value, ad.value

    def train_batch(self, states, actions, logp_old, returns, adv, b_div=None, apply_adam=True):
        s, a, l, r, v = (_f32(states), _f32(actions), _f32(logp_old), _f32(returns), _f32(adv))
        B = r.shape[0]
        grads = np.empty(self.nparam, np.float32)
        cd, ad, sk = C.c_float(), C.c_float(), C.c_int()
        self._chk(self.lib.wk_train_batch(
            self.h, int(B), float(B if b_div is None else b_div), _ptr(s), _ptr(a), _ptr(l),
            _ptr(r), _ptr(v), C.byref(cd), C.byref(ad), _ptr(grads), int(bool(apply_adam)),
            C.byref(sk)), "wk_train_batch")
        return grads, cd.value, ad.value, sk.value

    def minibatch_gradient(self, states, actions, logp_old, returns, adv, b_div=None):
        """The matrix-core minibatch gradient wk_ppo_update applies (no Adam)."""
        s, a, l, r, v = (_f32(states), _f32(actions), _f32(logp_old), _f32(returns), _f32(adv))
        B = r.shape[0]
        grads = np.empty(self.nparam, np.float32)
        cd, ad, sk = C.c_float(), C.c_float(), C.c_int()
        self._chk(self.lib.wk_minibatch_gradient(
            self.h, int(B), float(B if b_div is None else b_div), _ptr(s), _ptr(a), _ptr(l),
            _ptr(r), _ptr(v), C.byref(cd), C.byref(ad), _ptr(grads), C.byref(sk)),
            "wk_minibatch_gradient")
        return grads, cd.value, ad.value, sk.value

    # -- multi-GPU --
    @staticmethod
    def comm_unique_id():
        lib = load_library()
        buf = (C.c_uint8 * 128)()
        rc = lib.wk_comm_unique_id(buf)
        if rc != 0:
            raise WkError(f"wk_comm_unique_id failed: {lib.wk_last_error(None).decode()}")
        return bytes(buf)

    def comm_records(self, gather=None):
        """wk_comm_records, before comm_init / comm_init_host: the ranks exchange their statistics
        records, so TargetKL, LearnLogStd and reward normalisation run on any number of GPUs.
        gather=None: RCCL (then comm_init).  A callable (then comm_init_host) receives this rank's
        record, uint64[16], and returns every rank's, uint64[nranks, 16] in rank order
        (wk.dist.gather_records over torch.distributed); it is kept alive here.  A callback that
        raises, or returns another shape, fails the call in progress with WK_ERR_COMM: fatal for
        the whole job, like a failed all-reduce."""
        self._rx_error = None
        if gather is None:
            self._rx_fn = None
            self._chk(self.lib.wk_comm_records(self.h, None, None), "wk_comm_records")
            return

        def _cb(mine, out, user):
            try:
                n = getattr(self, "_nranks", 1)
                res = np.ascontiguousarray(gather(np.ctypeslib.as_array(mine, shape=(COMM_RECORD_WORDS,)).copy()),
                                           dtype=np.uint64)
                if res.shape != (n, COMM_RECORD_WORDS):
                    raise ValueError(f"the gather returned shape {res.shape}, not ({n}, {COMM_RECORD_WORDS})")
                np.ctypeslib.as_array(out, shape=(n, COMM_RECORD_WORDS))[:] = res
                return 0
            except Exception as ex:  # noqa: BLE001 -- reported as WK_ERR_COMM by the library
                self._rx_error = f"{type(ex).__name__}: {ex}"
                return 1
        self._rx_fn = HOST_ALLGATHER_FN(_cb)
        self._chk(self.lib.wk_comm_records(self.h, C.cast(self._rx_fn, C.c_void_p), None), "wk_comm_records")

    def comm_init(self, rank, nranks, uid):
        self._nranks = int(nranks)
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._chk(self.lib.wk_comm_init(self.h, int(rank), int(nranks), buf), "wk_comm_init")

    def comm_init_host(self, rank, nranks, allreduce):
        """wk_comm_init_host: `allreduce(np.ndarray float32 view)` sums the slab over ranks in
        place (e.g. torch.distributed over gloo); the callback object is kept alive here.
        A callback that raises fails this rank's wk_ppo_update with WK_ERR_COMM while the
        peers wait inside their own all-reduce: the WkError carries the exception's text and
        must be treated as fatal for the whole job (let it propagate so the launcher tears the
        process group down; the ranks' replicas have diverged)."""
        self._host_ar_error = None
        self._nranks = int(nranks)

        def _cb(buf, n, user):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(n,)))
                return 0
            except Exception as ex:  # noqa: BLE001 -- reported as WK_ERR_COMM by the library
                self._host_ar_error = f"{type(ex).__name__}: {ex}"
                return 1
        self._host_ar = HOST_ALLREDUCE_FN(_cb)
        self._chk(self.lib.wk_comm_init_host(self.h, int(rank), int(nranks), self._host_ar, None),
                  "wk_comm_init_host")

    def comm_ipc_handle(self):
        """wk_comm_ipc_handle: this rank's IPC_HANDLE_BYTES exchange record"""
        h = (C.c_uint8 * IPC_HANDLE_BYTES)()
        self._chk(self.lib.wk_comm_ipc_handle(self.h, h), "wk_comm_ipc_handle")
        return bytes(h)

    def comm_init_ipc_records(self, rank, nranks, records):
        """wk_comm_init_ipc with every rank's record (rank order)"""
        if len(records) != nranks or any(len(x) != IPC_HANDLE_BYTES for x in records):
            raise WkError(f"wk_comm_init_ipc: need one {IPC_HANDLE_BYTES}-byte record per rank")
        buf = (C.c_uint8 * (IPC_HANDLE_BYTES * nranks)).from_buffer_copy(b"".join(records))
        self._chk(self.lib.wk_comm_init_ipc(self.h, int(rank), int(nranks), buf),
                  "wk_comm_init_ipc")

    def comm_init_ipc(self, rank, nranks, allgather):
        """wk_comm_ipc_handle + wk_comm_init_ipc: the one-shot exchange over peer-mapped memory.
        `allgather(bytes) -> list of bytes` (rank order) exchanges the records over any control
        plane (e.g. torch.distributed.all_gather_object over gloo).  Every rank joins the
        all-gather even when its own handle failed (it sends b""), so the ranks' collectives
        stay paired; then every rank raises."""
        try:
            rec, why = self.comm_ipc_handle(), None
        except WkError as ex:
            rec, why = b"", str(ex)
        records = allgather(rec)
        if why is not None:
            raise WkError(why)
        bad = [r for r, x in enumerate(records) if len(x) != IPC_HANDLE_BYTES]
        if bad:
            raise WkError(f"wk_comm_init_ipc: rank(s) {bad} have no exchange record")
        self.comm_init_ipc_records(rank, nranks, records)

    def comm_set_timeout(self, seconds):
        """wk_comm_set_timeout: the IPC exchange's bounded peer wait (default 30 s, or
        WK_XCH_TIMEOUT_S at the mapping)"""
        self._chk(self.lib.wk_comm_set_timeout(self.h, float(seconds)), "wk_comm_set_timeout")

    COMM_KINDS = {0: "none", 1: "rccl", 2: "host", 3: "ipc"}

    def comm_info(self):
        """wk_comm_info: (exchange kind, whether the IPC region is uncached device memory)"""
        k, f = C.c_int(), C.c_int()
        self._chk(self.lib.wk_comm_info(self.h, C.byref(k), C.byref(f)), "wk_comm_info")
        return self.COMM_KINDS[k.value], bool(f.value & 1)

    # the reference's per-body call shape (Environment.StepObjects, Environment.cs:126-143)
    def take_actions(self, env, actions):
        """wk_take_actions: Walker.TakeActions for walker env (the next frame's torques)"""
        a = _f32(actions).reshape(4).copy()
        self._chk(self.lib.wk_take_actions(self.h, int(env), _ptr(a)), "wk_take_actions")

    def object_update(self, list_count, delta_time):
        """wk_object_update: one IObject.Update call; True when this call ran the frame's step"""
        r = self.lib.wk_object_update(self.h, int(list_count), float(delta_time))
        self._chk(min(r, 0), "wk_object_update")
        return r == 1

    def joint_step(self):
        self._chk(self.lib.wk_joint_step(self.h), "wk_joint_step")

    def body_order(self, env):
        """wk_body_order: walker env's body list as part ids (floor last in episode 0, first after
        a reset)"""
        parts, n = (C.c_int * 15)(), C.c_int()
        self._chk(self.lib.wk_body_order(self.h, int(env), parts, C.byref(n)), "wk_body_order")
        return list(parts[: n.value])

    def xch_profile(self, minibatches):
        """wk_comm_xch_profile: stamp the next exchange launches (a ring of `minibatches`; 0 off)"""
        self._chk(self.lib.wk_comm_xch_profile(self.h, int(minibatches)), "wk_comm_xch_profile")

    def xch_stamps(self, max_launches=1 << 16):
        """wk_comm_xch_stamps: uint64 [launches, blocks, 4] constant-clock ticks (10 ns) per block
        -- entry, slab published, peers' flags seen, exit -- for the last stamped launches"""
        import numpy as np
        n, b = C.c_int(), C.c_int()
        self._chk(self.lib.wk_comm_xch_stamps(self.h, None, 0, C.byref(n), C.byref(b)),
                  "wk_comm_xch_stamps")
        buf = np.zeros((max_launches, b.value, 4), np.uint64)
        self._chk(self.lib.wk_comm_xch_stamps(self.h, buf.ctypes.data, max_launches, C.byref(n),
                                              C.byref(b)), "wk_comm_xch_stamps")
        return buf[: n.value]

    def allreduce_test(self, x):
        x = _f32(x).copy()
        self._chk(self.lib.wk_allreduce_test(self.h, _ptr(x), x.size), "wk_allreduce_test")
        return x

    GRAD_KERNELS = {0: "k_ppo_grad_ws", 1: "k_ppo_grad_tp", 2: "k_ppo_grad_tp1",
                    3: "k_ppo_grad_mfma", 4: "k_net_grad"}

    def grad_kernel(self, minibatch=0):
        """wk_grad_kernel: the name of the gradient kernel the update launches at this per-GPU
        minibatch (0 = config Minibatch)"""
        k = self.lib.wk_grad_kernel(self.h, int(minibatch))
        self._chk(k if k < 0 else 0, "wk_grad_kernel")
        return self.GRAD_KERNELS[k]

    def time_gradient(self, minibatch=0, reps=64, per_launch_events=False):
        """wk_time_gradient_ex: mean ms of the update's gradient kernel over `reps` back-to-back
        launches on minibatch 0 of the current trajectory -- one event pair around the burst,
        or (per_launch_events) one around every launch, as profile level 2 times the update"""
        ms = C.c_double()
        self._chk(self.lib.wk_time_gradient_ex(self.h, int(minibatch), int(reps),
                                               int(bool(per_launch_events)), C.byref(ms)),
                  "wk_time_gradient_ex")
        return ms.value

    def rollout_mapping(self):
        """wk_rollout_mapping: {lanes_per_walker, walkers_per_wave, waves (holding walkers),
        waves_launched (the grid, whole 4-wave blocks for the split kernels)} of a rollout launch"""
        L, w = C.c_int(), C.c_int()
        n, nl = C.c_int64(), C.c_int64()
        self._chk(self.lib.wk_rollout_mapping(self.h, C.byref(L), C.byref(w), C.byref(n),
                                              C.byref(nl)), "wk_rollout_mapping")
        return {"lanes_per_walker": L.value, "walkers_per_wave": w.value, "waves": n.value,
                "waves_launched": nl.value}

    # -- counting replay / snapshots --
    def count_events(self, k):
        """wk_count_events: replay the last rollout's first k action rows through the
        counting kernel; returns the WK_NEV event totals (see include/wk_api.h)."""
        c = np.zeros(NEV, np.uint64)
        self._chk(self.lib.wk_count_events(self.h, int(k), _ptr(c)), "wk_count_events")
        return c

    def snapshot(self):
        self._chk(self.lib.wk_snapshot(self.h, 0), "wk_snapshot")

    def restore(self):
        self._chk(self.lib.wk_snapshot(self.h, 1), "wk_snapshot")

    # -- profiling --
    def profile_enable(self, on=True):
        """on: False/0 off, True/1 per rollout / update, 2 per kernel launch as well"""
        self._chk(self.lib.wk_profile_enable(self.h, int(on)), "wk_profile_enable")

    def profile_reset(self):
        self._chk(self.lib.wk_profile_reset(self.h), "wk_profile_reset")

    def profile(self):
        p = Profile()
        self._chk(self.lib.wk_profile_get(self.h, C.byref(p)), "wk_profile_get")
        return p.as_dict()
