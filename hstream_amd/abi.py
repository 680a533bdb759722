"""ctypes mirror of include/hstream_gpu.h (structs, enums, status codes).

Kept in one place so the product binding (``hstream_amd.engine``) and the test
oracle binding (``oracle/pyoracle.py``) describe the exact same ABI.
"""
import collections
import ctypes as C

HSG_OK = 0
HSG_E_INVALID = -1
HSG_E_OOM = -2
HSG_E_CAPACITY = -3
HSG_E_DEVICE = -4
HSG_E_COMM = -5
HSG_E_RANGE = -6

STATUS_NAMES = {
    HSG_OK: "HSG_OK",
    HSG_E_INVALID: "HSG_E_INVALID",
    HSG_E_OOM: "HSG_E_OOM",
    HSG_E_CAPACITY: "HSG_E_CAPACITY",
    HSG_E_DEVICE: "HSG_E_DEVICE",
    HSG_E_COMM: "HSG_E_COMM",
    HSG_E_RANGE: "HSG_E_RANGE",
}

HSG_KEY_NONE = 0xFFFFFFFF
HSG_VIEW_MAX_KEYS = 1024  # hsg_view_get
HSG_TRANSPORT_RCCL = 0
HSG_TRANSPORT_HOST = 1
HSG_COMM_ID_BYTES = 128
HSG_DEFAULT_GRACE_MS = 86400000

# hsg_window_kind
HSG_TUMBLING = 0
HSG_HOPPING = 1
HSG_SESSION = 2
HSG_UNWINDOWED = 3

# hsg_emit_mode
HSG_EMIT_PER_RECORD = 0
HSG_EMIT_PER_BATCH = 1
HSG_EMIT_NONE = 2

# hsg_col_type
HSG_I64 = 0
HSG_F64 = 1

# hsg_agg_kind
HSG_COUNT_ALL = 0
HSG_COUNT = 1
HSG_SUM = 2
HSG_MIN = 3
HSG_MAX = 4
HSG_AVG = 5
HSG_LAST = 6

# hsg_mem
HSG_MEM_HOST = 0
HSG_MEM_DEVICE = 1

# narrow transport encodings (hsg_batch ts_enc / col_enc)
HSG_ENC_FULL = 0
HSG_ENC_TS32 = 1
HSG_ENC_I32 = 2
HSG_ENC_DEC32 = 3
HSG_ENC_K16 = 4
HSG_ENC_TS16 = 5
HSG_TS16_FRAME = 4096
# hsg_batch_narrow / hsg_decode_json_batch: encodings the consumer accepts (hstream_ingest.h)
HSG_NARROW_K16 = 1
HSG_NARROW_TS16 = 2
HSG_NARROW_TS32 = 4
HSG_NARROW_I32 = 8
HSG_NARROW_DEC32 = 16
HSG_NARROW_ALL = 31

# hsg_op_config.flags
HSG_OPF_LITERAL_FORMS = 1


# hsg_where_opcode: the WHERE program an op runs on the GPU ahead of its aggregate
HSG_W_COL = 0
HSG_W_I64 = 1
HSG_W_F64 = 2
HSG_W_ADD = 3
HSG_W_SUB = 4
HSG_W_MUL = 5
HSG_W_EQ = 6
HSG_W_NE = 7
HSG_W_LT = 8
HSG_W_GT = 9
HSG_W_LE = 10
HSG_W_GE = 11
HSG_W_BETWEEN = 12
HSG_W_AND = 13
HSG_W_OR = 14
HSG_W_NOT = 15
HSG_W_FN = 32  # value -> value: the numeric function `arg` (hsg_fn); 16..31 are not opcodes
HSG_WHERE_MAX_INS = 64
HSG_WHERE_MAX_DEPTH = 8

# hsg_fn: the reference's numeric unary functions (unaryOpOnValue, Internal/Codegen.hs:139-179)
HSG_FN_NAMES = ["SIN", "SINH", "ASIN", "ASINH", "COS", "COSH", "ACOS", "ACOSH", "TAN", "TANH", "ATAN", "ATANH",
                "ABS", "CEIL", "FLOOR", "ROUND", "SQRT", "SIGN", "LOG", "LOG2", "LOG10", "EXP"]
(HSG_FN_SIN, HSG_FN_SINH, HSG_FN_ASIN, HSG_FN_ASINH, HSG_FN_COS, HSG_FN_COSH, HSG_FN_ACOS, HSG_FN_ACOSH,
 HSG_FN_TAN, HSG_FN_TANH, HSG_FN_ATAN, HSG_FN_ATANH, HSG_FN_ABS, HSG_FN_CEIL, HSG_FN_FLOOR, HSG_FN_ROUND,
 HSG_FN_SQRT, HSG_FN_SIGN, HSG_FN_LOG, HSG_FN_LOG2, HSG_FN_LOG10, HSG_FN_EXP) = range(22)
HSG_FN_COUNT = 22
# the exact family (function class 1); every other function is class 2
HSG_FN_EXACT = (HSG_FN_ABS, HSG_FN_CEIL, HSG_FN_FLOOR, HSG_FN_ROUND, HSG_FN_SQRT, HSG_FN_SIGN)
# ... whose result has the operand's type / is an i64; the rest give an f64
HSG_FN_KEEP_TYPE = (HSG_FN_ABS, HSG_FN_CEIL, HSG_FN_FLOOR, HSG_FN_ROUND)


class hsg_where_imm(C.Union):
    _fields_ = [("i", C.c_int64), ("f", C.c_double)]


class hsg_where_ins(C.Structure):
    _fields_ = [("op", C.c_int32), ("arg", C.c_int32), ("imm", hsg_where_imm)]


def where_ins(op, arg=0):
    """One instruction: where_ins(HSG_W_COL, c), where_ins(HSG_W_I64, int),
    where_ins(HSG_W_F64, float), where_ins(HSG_W_FN, HSG_FN_ABS),
    where_ins(HSG_W_ADD) ..."""
    ins = hsg_where_ins(op=int(op), arg=0)
    if op == HSG_W_COL or op == HSG_W_FN:
        ins.arg = int(arg)
    elif op == HSG_W_I64:
        ins.imm.i = int(arg)
    elif op == HSG_W_F64:
        ins.imm.f = float(arg)
    return ins


def where_array(program):
    """A program -- hsg_where_ins, or (op,) / (op, arg) tuples -- as a C array."""
    items = [p if isinstance(p, hsg_where_ins) else where_ins(*p) for p in program]
    return (hsg_where_ins * max(1, len(items)))(*items), len(items)


# computed columns (hsg_op_create_mapped): value programs over the batch's columns
HSG_MAP_STRICT = 1
HSG_MAP_MAX_EXPRS = 8
HSG_MAP_MAX_INS = 64


class hsg_map_expr(C.Structure):
    _fields_ = [("prog", C.POINTER(hsg_where_ins)), ("n", C.c_int32), ("flags", C.c_uint32)]


class hsg_map_stats(C.Structure):
    _fields_ = [
        ("map_dropped", C.c_uint64),
        ("map_dropped_total", C.c_uint64),
        ("computed_cols", C.c_uint32),
        ("aliased_cols", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class MapExpr(collections.namedtuple("MapExpr", "prog flags")):
    """One expression of a map: its value program -- hsg_where_ins, or (op,) /
    (op, arg) tuples -- and its flags (HSG_MAP_STRICT)."""

    __slots__ = ()

    def __new__(cls, prog, flags=0):
        return super().__new__(cls, list(prog), int(flags))


def _map_expr(e):
    """A map entry as a MapExpr: one already, or a bare program (flags 0)."""
    return e if isinstance(e, MapExpr) else MapExpr(e)


def map_expr_type(e, col_types):
    """The static type of a (well-formed) map expression, as hsg_map_check
    types it: ADD / SUB / MUL give an f64 iff an operand is one; of the
    functions SIGN gives an i64, ABS / CEIL / FLOOR / ROUND the operand's
    type, every other an f64 (include/hstream_gpu.h)."""
    prog, _ = _map_expr(e)
    st = []
    for p in prog:
        op, arg = (p.op, p.arg) if isinstance(p, hsg_where_ins) else (p[0], p[1] if len(p) > 1 else 0)
        if op == HSG_W_COL:
            st.append(0 <= arg < len(col_types) and col_types[arg] == HSG_F64)
        elif op in (HSG_W_I64, HSG_W_F64):
            st.append(op == HSG_W_F64)
        elif op == HSG_W_FN:
            x = st.pop() if st else False
            st.append(x if arg in HSG_FN_KEEP_TYPE else arg != HSG_FN_SIGN)
        else:
            r, l = (st.pop() if st else False), (st.pop() if st else False)
            st.append(l or r)
    return HSG_F64 if st and st[-1] else HSG_I64


def map_array(exprs):
    """A map -- a list of MapExpr, or of bare programs (flags 0) -- as a C
    array of hsg_map_expr. Returns (array, n_exprs, keepalive)."""
    keep, items = [], []
    for e in exprs:
        prog, flags = _map_expr(e)
        arr, n = where_array(prog)
        keep.append(arr)
        items.append(hsg_map_expr(prog=C.cast(arr, C.POINTER(hsg_where_ins)), n=n, flags=int(flags)))
    return (hsg_map_expr * max(1, len(items)))(*items), len(items), keep


class hsg_select_config(C.Structure):
    """A select op (hsg_op_create_select): the batch's columns, the changelog's room, the flags."""

    _fields_ = [
        ("n_cols", C.c_int32),
        ("flags", C.c_uint32),
        ("col_types", C.POINTER(C.c_int32)),
        ("out_capacity", C.c_uint64),
    ]


class hsg_select_stats(C.Structure):
    _fields_ = [
        ("where_dropped", C.c_uint64),
        ("where_dropped_total", C.c_uint64),
        ("expr_dropped", C.c_uint64),
        ("expr_dropped_total", C.c_uint64),
        ("having_dropped", C.c_uint64),
        ("having_dropped_total", C.c_uint64),
        ("emitted", C.c_uint64),
        ("emitted_total", C.c_uint64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class hsg_engine_config(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("rank", C.c_int32),
        ("nranks", C.c_int32),
        ("transport", C.c_int32),
        ("comm_id", C.POINTER(C.c_uint8)),
        ("batch_capacity", C.c_uint64),
    ]


class hsg_agg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("column", C.c_int32)]


class hsg_op_config(C.Structure):
    _fields_ = [
        ("window_kind", C.c_int32),
        ("emit_mode", C.c_int32),
        ("size_ms", C.c_int64),
        ("advance_ms", C.c_int64),
        ("gap_ms", C.c_int64),
        ("grace_ms", C.c_int64),
        ("n_cols", C.c_int32),
        ("n_aggs", C.c_int32),
        ("col_types", C.POINTER(C.c_int32)),
        ("aggs", C.POINTER(hsg_agg)),
        ("state_capacity", C.c_uint64),
        ("out_capacity", C.c_uint64),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class hsg_batch(C.Structure):
    _fields_ = [
        ("n", C.c_uint64),
        ("mem", C.c_int32),
        ("n_cols", C.c_int32),
        ("key_id", C.c_void_p),
        ("ts", C.c_void_p),
        ("cols", C.POINTER(C.c_void_p)),
        ("valid", C.POINTER(C.c_void_p)),
        ("ready_event", C.c_void_p),
        ("ts_enc", C.c_int32),
        ("key_enc", C.c_int32),
        ("ts_base", C.c_int64),
        ("col_enc", C.c_uint8 * 8),
        ("col_scale", C.c_uint8 * 8),
        ("ts_frames", C.c_void_p),
    ]


class hsg_decode_buffers(C.Structure):
    _fields_ = [
        ("capacity", C.c_uint64),
        ("key_id", C.c_void_p),
        ("ts", C.c_void_p),
        ("ts_frames", C.c_void_p),
        ("cols", C.POINTER(C.c_void_p)),
        ("valid", C.POINTER(C.c_void_p)),
        ("allow", C.c_uint32),
        ("reserved", C.c_uint32),
        ("col_ptrs", C.c_void_p * 8),
        ("valid_ptrs", C.c_void_p * 8),
    ]


class hsg_rows(C.Structure):
    _fields_ = [
        ("capacity", C.c_uint64),
        ("mem", C.c_int32),
        ("n_aggs", C.c_int32),
        ("key_id", C.c_void_p),
        ("win_start", C.c_void_p),
        ("win_end", C.c_void_p),
        ("src_index", C.c_void_p),
        ("aggs", C.POINTER(C.c_void_p)),
        ("form", C.c_void_p),
    ]


class hsg_probe(C.Structure):
    """The stream side of hsg_table_join: one poll batch's keys, arrival order."""

    _fields_ = [
        ("n", C.c_uint64),
        ("mem", C.c_int32),
        ("reserved", C.c_int32),
        ("key_id", C.c_void_p),
        ("ready_event", C.c_void_p),
    ]


class hsg_stats(C.Structure):
    _fields_ = [
        ("batches", C.c_uint64),
        ("records", C.c_uint64),
        ("records_owned", C.c_uint64),
        ("pairs", C.c_uint64),
        ("late_dropped", C.c_uint64),
        ("touched", C.c_uint64),
        ("state_rows", C.c_uint64),
        ("pending_rows", C.c_uint64),
        ("last_batch_ms", C.c_double),
        ("agg_kernel_ms", C.c_double),
        ("agg_kernel_launches", C.c_uint64),
        ("exchange_ms", C.c_double),
        ("exchange_bytes", C.c_uint64),
        ("pairs_total", C.c_uint64),
        ("touched_total", C.c_uint64),
        ("state_slots", C.c_uint64),
        ("state_row_bytes", C.c_uint64),
        ("spilled_rows", C.c_uint64),
        ("spill_events", C.c_uint64),
        ("table_slots", C.c_uint64),
        ("grow_events", C.c_uint64),
        ("lean_batches", C.c_uint64),
        ("direct_batches", C.c_uint64),
        ("replays", C.c_uint64),
        ("overflow_rows", C.c_uint64),
        ("overflow_rebuilds", C.c_uint64),
        ("where_dropped", C.c_uint64),
        ("where_dropped_total", C.c_uint64),
        ("having_dropped", C.c_uint64),
        ("having_dropped_total", C.c_uint64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# Every symbol include/hstream_gpu.h declares (checked by tests/test_abi.py).
EXPORTED_SYMBOLS = [
    "hsg_comm_unique_id",
    "hsg_engine_create",
    "hsg_engine_destroy",
    "hsg_engine_last_error",
    "hsg_op_create",
    "hsg_where_check",
    "hsg_op_create_where",
    "hsg_having_check",
    "hsg_op_create_filtered",
    "hsg_having_tile_rows",
    "hsg_map_check",
    "hsg_op_create_mapped",
    "hsg_op_map_stats",
    "hsg_map_grid_threads",
    "hsg_prog_fn_class",
    "hsg_map_grid_threads_fn",
    "hsg_select_check",
    "hsg_op_create_select",
    "hsg_op_select_stats",
    "hsg_select_tile_rows",
    "hsg_select_grid_groups",
    "hsg_op_destroy",
    "hsg_op_reset",
    "hsg_last_error",
    "hsg_push_batch",
    "hsg_push_batch_async",
    "hsg_op_wait",
    "hsg_pending_rows",
    "hsg_drain",
    "hsg_op_set_changelog",
    "hsg_state_rows",
    "hsg_dump_state",
    "hsg_view_get",
    "hsg_table_join",
    "hsg_table_join_tile",
    "hsg_op_stats",
    "hsg_testing_set_knob",
]

# testing knobs (hsg_testing_set_knob)
HSG_KNOB_XPART_LOG2 = 1
HSG_KNOB_SESS_ARENA_MIN = 2
HSG_KNOB_X_CLASSIC = 3


# Every symbol include/hstream_ingest.h declares (host ingest, no GPU needed).
INGEST_SYMBOLS = [
    "hsg_keydict_create",
    "hsg_keydict_destroy",
    "hsg_keydict_size",
    "hsg_keydict_encode",
    "hsg_keydict_find",
    "hsg_keydict_text",
    "hsg_keydict_spelling_text",
    "hsg_decoder_create",
    "hsg_decoder_destroy",
    "hsg_batch_narrow",
    "hsg_decode_json_batch",
    "hsg_decode_json",
    "hsg_decode_json_spelled",
    "hsg_gpu_decoder_create",
    "hsg_gpu_decode_json",
    "hsg_gpu_decoder_fetch",
    "hsg_gpu_decoder_destroy",
    "hsg_gpu_decoder_last_error",
    "hsg_json_fast_probe",
]

# device decode limits (hstream_ingest.h "GPU ingest")
HSG_GPU_DEC_MAX_RECORD = 4096
HSG_GPU_DEC_MAX_KEY = 48
HSG_GPU_DEC_MAX_COLS = 8
HSG_GPU_DEC_MAX_NAME = 64

HSG_SPELL_ALT = 0x80000000

# hsg_decode_status
HSG_DEC_OK = 0
HSG_DEC_NOT_OBJECT = 1
HSG_DEC_NO_KEY = 2
HSG_DEC_TYPE = 3
HSG_DEC_NOT_INTEGRAL = 4
HSG_DEC_RANGE = 5


class hsg_decoder_config(C.Structure):
    _fields_ = [
        ("key_field", C.c_char_p),
        ("n_cols", C.c_int32),
        ("col_fields", C.POINTER(C.c_char_p)),
        ("col_types", C.POINTER(C.c_int32)),
        ("col_numeric", C.POINTER(C.c_uint8)),
        ("literal_forms", C.c_int32),
    ]


class hsg_gpu_decode_stats(C.Structure):
    _fields_ = [
        ("records", C.c_uint64),
        ("accepted", C.c_uint64),
        ("host_records", C.c_uint64),
        ("new_keys", C.c_uint64),
        ("table_slots", C.c_uint64),
        ("table_rebuilds", C.c_uint64),
    ]


class hsg_json_probe(C.Structure):
    _fields_ = [
        ("accept", C.c_int32),
        ("key_tag", C.c_int32),
        ("key_neg", C.c_int32),
        ("key_e", C.c_int32),
        ("key_m", C.c_uint64),
        ("key_off", C.c_uint32),
        ("key_len", C.c_uint32),
        ("key_int_form", C.c_int32),
        ("reserved", C.c_int32),
        ("words", C.c_uint64 * 8),
        ("valid", C.c_uint8 * 8),
    ]


class hsg_sink_config(C.Structure):
    _fields_ = [
        ("windowed", C.c_int32),
        ("n_members", C.c_int32),
        ("key_field", C.c_char_p),
        ("aliases", C.POINTER(C.c_char_p)),
        ("agg_index", C.POINTER(C.c_int32)),
    ]


class hsg_sink_spellings(C.Structure):
    _fields_ = [
        ("spell", C.c_void_p),
        ("n", C.c_uint64),
        ("src_base", C.c_int64),
        ("mem", C.c_int32),
        ("reserved", C.c_int32),
    ]


class hsg_sink_records(C.Structure):
    _fields_ = [
        ("mem", C.c_int32),
        ("reserved0", C.c_int32),
        ("key_capacity", C.c_uint64),
        ("value_capacity", C.c_uint64),
        ("key_bytes", C.c_void_p),
        ("key_off", C.c_void_p),
        ("value_bytes", C.c_void_p),
        ("value_off", C.c_void_p),
    ]



# Every symbol include/hstream_sink.h declares.
SINK_SYMBOLS = ["hsg_sink_create", "hsg_sink_destroy", "hsg_sink_encode", "hsg_sink_encode_spelled",
                "hsg_sink_member_order", "hsg_format_number"]


class hsg_join_config(C.Structure):
    _fields_ = [("before_ms", C.c_int64), ("after_ms", C.c_int64), ("batch_capacity", C.c_uint64)]


class hsg_join_batch(C.Structure):
    _fields_ = [
        ("n", C.c_uint64),
        ("mem", C.c_int32),
        ("reserved0", C.c_int32),
        ("side", C.c_void_p),
        ("key_id", C.c_void_p),
        ("join_key", C.c_void_p),
        ("ts", C.c_void_p),
        ("handle", C.c_void_p),
    ]


class hsg_join_rows(C.Structure):
    _fields_ = [
        ("capacity", C.c_uint64),
        ("mem", C.c_int32),
        ("reserved0", C.c_int32),
        ("this_handle", C.c_void_p),
        ("other_handle", C.c_void_p),
        ("join_key", C.c_void_p),
        ("ts", C.c_void_p),
    ]


HSG_JOIN_MAX_COLS = 8


class hsg_join_values(C.Structure):
    _fields_ = [("n_cols", C.c_int32 * 2), ("col_types", (C.c_int32 * 8) * 2)]


class hsg_join_cols(C.Structure):
    _fields_ = [("cols", C.POINTER(C.c_void_p)), ("valid", C.POINTER(C.c_void_p))]


class hsg_join_joined(C.Structure):
    _fields_ = [
        ("capacity", C.c_uint64),
        ("mem", C.c_int32),
        ("key_col", C.c_int32),
        ("key_id", C.c_void_p),
        ("ts", C.c_void_p),
        ("cols", C.POINTER(C.c_void_p)),
        ("valid", C.POINTER(C.c_void_p)),
        ("this_handle", C.c_void_p),
        ("other_handle", C.c_void_p),
        ("join_key", C.c_void_p),
    ]


# Every symbol include/hstream_join.h declares.
JOIN_SYMBOLS = ["hsg_join_create", "hsg_join_destroy", "hsg_join_last_error", "hsg_join_push", "hsg_join_pending",
                "hsg_join_drain", "hsg_join_state_rows", "hsg_join_create_valued", "hsg_join_push_valued",
                "hsg_join_drain_batch", "hsg_join_value_rows", "hsg_join_value_stride"]


# void (*hsg_done_fn)(void *ctx, int rc)
HSG_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int)


class HStreamGpuError(RuntimeError):
    """Raised for a negative status; mirrors the reference's HStreamError (Error.hs:11-18)."""

    def __init__(self, status, message=""):
        self.status = status
        name = STATUS_NAMES.get(status, str(status))
        super().__init__(f"{name}: {message}" if message else name)


def agg_output_is_f64(kind, col_type):
    if kind in (HSG_COUNT_ALL, HSG_COUNT):
        return False
    if kind == HSG_AVG:
        return True
    return col_type == HSG_F64
