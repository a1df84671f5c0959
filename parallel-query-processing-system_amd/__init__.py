"""ctypes binding of the MI355X SELECT/WHERE backend (libpqps_hip.so).

The product is C: `csrc/pqps_hip.hip` (kernels + C-ABI shim, include/pqps_hip.h)
and the C11 engine under `engine/hip/` + `host/` (include/executeEngine-hip.h).
This module only mirrors those headers for Python callers (tests, bench.py);
it contains no compute and no fallback: if the shared library is missing or
no GPU is visible, calls fail loudly.

The directory name contains '-', so import it with::

    import importlib.util, sys
    spec = importlib.util.spec_from_file_location(
        "pqps_amd", "<repo>/parallel-query-processing-system_amd/__init__.py")
    pqps_amd = importlib.util.module_from_spec(spec); sys.modules["pqps_amd"] = pqps_amd
    spec.loader.exec_module(pqps_amd)
"""
from __future__ import annotations

import ctypes as C
import os
import pathlib
import subprocess

PKG_DIR = pathlib.Path(__file__).resolve().parent
# (PQPS_LIB: a development build of the same library, e.g. -DPQPS_DEV_SHAPES / -DPQPS_STAMPS, for tuning runs)
LIB_PATH = pathlib.Path(os.environ.get("PQPS_LIB") or (PKG_DIR / "libpqps_hip.so"))

MAX_COLUMNS = 12
MAX_LEAVES = 32
TT_LEAVES = 6
TILE_ROWS = 4096
SLOT_HEADER_WORDS = 4
ACCEPT, REJECT = 0xFE, 0xFF
WIDTH_BITS = 0x81                  # pqps_column.width of a bit plane (PQPS_WIDTH_BITS)
WIDTH_P12 = 0x8C                   # ... of a 12-bit packed copy of a u16 column (PQPS_WIDTH_P12)
HIPKIND_U64, HIPKIND_I32, HIPKIND_BOOL, HIPKIND_DICT = 0, 1, 2, 3     # include/hipPredicate.h
MEMBER_BITMAP, MEMBER_LIST = 0, 1  # pqps_member_flags: lookup form ...
MEMBER_BYTES, MEMBER_PLANE = 0, 1  # ... and output form
REMAP_LDS, REMAP_GLOBAL = 0, 1     # pqps_remap_codes: where the lookups go
REMAP_LDS_CODES = 4096             # a table of up to this many codes is staged into LDS
MEMBER_LDS_BITS = 1 << 18          # a bitmap of up to this many bits is staged into LDS
MEMBER_MAX_RUNS, MEMBER_MAX_ITEMS = 4, 65536
SYNTH_USERS = 2000
COMPACT_TILE = 1024                # PQPS_COMPACT_TILE: bins one wave of pqps_bins_compact takes
WIDE_COUNT_SLOTS = 8192            # PQPS_WIDE_COUNT_SLOTS / PQPS_WIDE_VALUE_SLOTS: the LDS front of the wide bins
WIDE_VALUE_SLOTS = 2048
TOP_BY = {"key": 0, "count": 1, "sum": 2, "min": 3, "max": 4}           # HIPTOP_BY_*
TOP_BINS_BUDGET = 256 << 20        # HIP_TOP_BINS_BUDGET

COLUMNS = ["command_id", "raw_command", "base_command", "shell_type", "exit_code", "timestamp",
           "sudo_used", "working_directory", "user_id", "user_name", "host_name", "risk_level"]
COL = {name: i for i, name in enumerate(COLUMNS)}
KIND_U64, KIND_I32, KIND_BOOL, KIND_DICT = 0, 1, 2, 3
COLUMN_KIND = [KIND_U64, KIND_DICT, KIND_DICT, KIND_DICT, KIND_I32, KIND_DICT,
               KIND_BOOL, KIND_DICT, KIND_I32, KIND_DICT, KIND_DICT, KIND_I32]
FIELD_UINT64, FIELD_INT, FIELD_STRING, FIELD_BOOL = 0, 1, 2, 3
DEFAULT_INDEXES = [("command_id", 0), ("user_id", 1), ("risk_level", 1), ("exit_code", 1), ("sudo_used", 3)]


# ---- include/logType.h, include/executeEngine-serial.h ---------------------
class Record(C.Structure):
    _fields_ = [
        ("command_id", C.c_ulonglong),
        ("raw_command", C.c_char * 512),
        ("base_command", C.c_char * 100),
        ("shell_type", C.c_char * 20),
        ("exit_code", C.c_int),
        ("timestamp", C.c_char * 30),
        ("sudo_used", C.c_bool),
        ("working_directory", C.c_char * 200),
        ("user_id", C.c_int),
        ("user_name", C.c_char * 50),
        ("host_name", C.c_char * 100),
        ("risk_level", C.c_int),
    ]


class WhereClause(C.Structure):
    pass


WhereClause._fields_ = [
    ("attribute", C.c_char_p),
    ("operator", C.c_char_p),
    ("value", C.c_char_p),
    ("value_type", C.c_int),
    ("next", C.POINTER(WhereClause)),
    ("logical_op", C.c_char_p),
    ("sub", C.POINTER(WhereClause)),
]


class ResultSet(C.Structure):
    _fields_ = [
        ("numRecords", C.c_int),
        ("numColumns", C.c_int),
        ("columnNames", C.POINTER(C.c_char_p)),
        ("columnTypes", C.POINTER(C.c_int)),
        ("data", C.POINTER(C.POINTER(C.c_char_p))),
        ("queryTime", C.c_double),
        ("success", C.c_bool),
    ]


class ColumnarResult(C.Structure):
    """struct hipColumnarResult (include/executeEngine-hip.h)."""
    _fields_ = [("numRecords", C.c_int), ("numColumns", C.c_int), ("columnNames", C.POINTER(C.c_char_p)),
                ("columnKinds", C.POINTER(C.c_int)), ("values", C.POINTER(C.c_void_p)),
                ("dictionaries", C.POINTER(C.POINTER(C.c_char_p))), ("dictionarySizes", C.POINTER(C.c_int)),
                ("queryTime", C.c_double), ("success", C.c_bool)]


class GroupResult(C.Structure):
    """struct hipGroupResult (include/executeEngine-hip.h)."""
    _fields_ = [("column", C.c_int), ("kind", C.c_int), ("numGroups", C.c_int), ("total", C.c_longlong),
                ("keys", C.POINTER(C.c_longlong)), ("keyText", C.POINTER(C.c_char_p)),
                ("counts", C.POINTER(C.c_ulonglong)), ("queryTime", C.c_double), ("success", C.c_bool)]


class AggregateResult(C.Structure):
    """struct hipAggregateResult (include/executeEngine-hip.h)."""
    _fields_ = [("valueColumn", C.c_int), ("valueKind", C.c_int), ("groupColumn", C.c_int), ("groupKind", C.c_int),
                ("numGroups", C.c_int), ("total", C.c_longlong),
                ("keys", C.POINTER(C.c_longlong)), ("keyText", C.POINTER(C.c_char_p)), ("counts", C.POINTER(C.c_ulonglong)),
                ("sums", C.POINTER(C.c_longlong)), ("mins", C.POINTER(C.c_longlong)), ("maxs", C.POINTER(C.c_longlong)),
                ("queryTime", C.c_double), ("success", C.c_bool)]


class BucketResult(C.Structure):
    """struct hipBucketResult (include/executeEngine-hip.h)."""
    _fields_ = [("groupColumn", C.c_int), ("groupKind", C.c_int), ("bucketMode", C.c_int), ("bucketArg", C.c_longlong),
                ("valueColumn", C.c_int), ("valueKind", C.c_int), ("numGroups", C.c_int), ("total", C.c_longlong),
                ("keys", C.POINTER(C.c_longlong)), ("keyText", C.POINTER(C.c_char_p)), ("counts", C.POINTER(C.c_ulonglong)),
                ("sums", C.POINTER(C.c_longlong)), ("mins", C.POINTER(C.c_longlong)), ("maxs", C.POINTER(C.c_longlong)),
                ("queryTime", C.c_double), ("success", C.c_bool)]


class GroupPairResult(C.Structure):
    """struct hipGroupPairResult (include/executeEngine-hip.h)."""
    _fields_ = [("groupColumn", C.c_int * 2), ("groupKind", C.c_int * 2), ("valueColumn", C.c_int), ("valueKind", C.c_int),
                ("numGroups", C.c_int), ("total", C.c_longlong),
                ("keys", C.POINTER(C.c_longlong) * 2), ("keyText", C.POINTER(C.c_char_p) * 2), ("counts", C.POINTER(C.c_ulonglong)),
                ("sums", C.POINTER(C.c_longlong)), ("mins", C.POINTER(C.c_longlong)), ("maxs", C.POINTER(C.c_longlong)),
                ("queryTime", C.c_double), ("success", C.c_bool)]


class GroupTopResult(C.Structure):
    """struct hipGroupTopResult (include/executeEngine-hip.h)."""
    _fields_ = [("groupColumn", C.c_int), ("groupKind", C.c_int), ("valueColumn", C.c_int), ("valueKind", C.c_int),
                ("orderBy", C.c_int), ("descending", C.c_bool), ("limit", C.c_longlong), ("numGroups", C.c_int),
                ("groupsTotal", C.c_longlong), ("total", C.c_longlong),
                ("keys", C.POINTER(C.c_longlong)), ("keyText", C.POINTER(C.c_char_p)), ("counts", C.POINTER(C.c_ulonglong)),
                ("sums", C.POINTER(C.c_longlong)), ("mins", C.POINTER(C.c_longlong)), ("maxs", C.POINTER(C.c_longlong)),
                ("queryTime", C.c_double), ("success", C.c_bool)]


class SetHaving(C.Structure):
    """struct hipSetHaving (include/executeEngine-hip.h)."""
    _fields_ = [("aggregate", C.c_int), ("valueColumn", C.c_char_p), ("op", C.c_char_p), ("constant", C.c_char_p)]


class ValueSetResult(C.Structure):
    """struct hipValueSet (include/executeEngine-hip.h)."""
    _fields_ = [("success", C.c_bool), ("id", C.c_uint), ("column", C.c_int), ("kind", C.c_int),
                ("members", C.c_ulonglong), ("rows", C.c_ulonglong), ("queryTime", C.c_double)]


class SetKeysResult(C.Structure):
    """struct hipSetKeys (include/executeEngine-hip.h)."""
    _fields_ = [("success", C.c_bool), ("column", C.c_int), ("kind", C.c_int), ("numKeys", C.c_int),
                ("keys", C.POINTER(C.c_longlong)), ("keyText", C.POINTER(C.c_char_p))]


class SetInfo(C.Structure):
    """struct hipSetInfo (include/hipPredicate.h)."""
    _fields_ = [("id", C.c_uint32), ("column", C.c_int), ("kind", C.c_int), ("base", C.c_uint32), ("n_bits", C.c_uint64),
                ("members", C.c_uint64), ("stale", C.c_int)]


class Having(C.Structure):
    """struct hipHaving (include/hipPredicate.h)."""
    _fields_ = [("field", C.c_int), ("op", C.c_int), ("constant", C.c_uint64), ("value_signed", C.c_int)]


class DistinctResult(C.Structure):
    """struct hipDistinctResult (include/executeEngine-hip.h)."""
    _fields_ = [("valueColumn", C.c_int), ("valueKind", C.c_int), ("groupColumn", C.c_int), ("groupKind", C.c_int),
                ("numGroups", C.c_int), ("total", C.c_longlong),
                ("keys", C.POINTER(C.c_longlong)), ("keyText", C.POINTER(C.c_char_p)), ("distinct", C.POINTER(C.c_ulonglong)),
                ("queryTime", C.c_double), ("success", C.c_bool)]


class GroupFirstResult(C.Structure):
    """struct hipGroupFirstResult (include/executeEngine-hip.h)."""
    _fields_ = [("groupColumn", C.c_int), ("groupKind", C.c_int), ("orderColumn", C.c_int), ("orderKind", C.c_int),
                ("descending", C.c_bool), ("numGroups", C.c_int), ("total", C.c_longlong),
                ("keys", C.POINTER(C.c_longlong)), ("keyText", C.POINTER(C.c_char_p)), ("rows", C.POINTER(C.c_uint)),
                ("orderKeys", C.POINTER(C.c_longlong)), ("orderText", C.POINTER(C.c_char_p)),
                ("queryTime", C.c_double), ("success", C.c_bool)]


class GroupHeadResult(C.Structure):
    """struct hipGroupHeadResult (include/executeEngine-hip.h)."""
    _fields_ = [("groupColumn", C.c_int), ("groupKind", C.c_int), ("orderColumn", C.c_int), ("orderKind", C.c_int),
                ("descending", C.c_bool), ("limit", C.c_int), ("numGroups", C.c_int), ("total", C.c_longlong),
                ("keys", C.POINTER(C.c_longlong)), ("keyText", C.POINTER(C.c_char_p)), ("offsets", C.POINTER(C.c_longlong)),
                ("rows", C.POINTER(C.c_uint)), ("orderKeys", C.POINTER(C.c_longlong)), ("orderText", C.POINTER(C.c_char_p)),
                ("queryTime", C.c_double), ("success", C.c_bool)]


class HeadList(C.Structure):
    """struct hipHeadList (include/hipPredicate.h)."""
    _fields_ = [("n", C.c_uint64), ("bins", C.POINTER(C.c_uint32)), ("words", C.POINTER(C.c_uint64)), ("best", C.POINTER(C.c_uint64))]


HEAD_ROUNDS_MAX = 16        # PQPS_HEAD_ROUNDS_MAX (include/pqps_hip.h)


class QuantileResult(C.Structure):
    """struct hipQuantileResult (include/executeEngine-hip.h)."""
    _fields_ = [("valueColumn", C.c_int), ("valueKind", C.c_int), ("groupColumn", C.c_int), ("groupKind", C.c_int),
                ("numGroups", C.c_int), ("numFractions", C.c_int), ("passes", C.c_int), ("total", C.c_longlong),
                ("keyText", C.POINTER(C.c_char_p)), ("counts", C.POINTER(C.c_ulonglong)), ("values", C.POINTER(C.c_longlong)),
                ("valueText", C.POINTER(C.c_char_p)), ("queryTime", C.c_double), ("success", C.c_bool)]


QUANTILE_PPM = 1_000_000                                     # HIPQUANTILE_PPM (include/hipPredicate.h)
QUANTILE_MAX_FRACTIONS = 16                                  # HIPQUANTILE_MAX_FRACTIONS
DIGIT_BITS_MAX, DIGIT_SLOTS_MAX, DIGIT_WORDS_MAX = 11, 16, 1 << 22   # PQPS_DIGIT_* (include/pqps_hip.h)


class ColumnData(C.Structure):
    """struct hipColumnData (include/executeEngine-hip.h)."""
    _fields_ = [("values", C.c_void_p), ("width", C.c_uint), ("on_device", C.c_int),
                ("dictionary", C.POINTER(C.c_char_p)), ("dictionary_count", C.c_int)]


class DeviceResult(C.Structure):
    """struct hipDeviceResult (include/executeEngine-hip.h)."""
    _fields_ = [("count", C.c_longlong), ("ids_dev", C.c_void_p), ("device", C.c_int), ("n_shards", C.c_int),
                ("shard_count", C.c_ulonglong * 16)]


class BenchResult(C.Structure):
    """struct hipBenchResult (include/engineBench.h)."""
    _fields_ = [("seconds", C.c_double), ("queries", C.c_longlong), ("matches", C.c_longlong), ("mismatches", C.c_longlong),
                ("issue_seconds", C.c_double), ("await_seconds", C.c_double),
                ("want_checksum", C.c_int), ("have_checksum", C.c_int), ("checksum", C.c_ulonglong * 2),
                ("keep_last", C.c_int), ("last_ticket", C.c_void_p)]


class EngineS(C.Structure):
    _fields_ = [
        ("tableName", C.c_char_p),
        ("bplus_tree_roots", C.c_void_p),
        ("num_indexes", C.c_int),
        ("indexed_attributes", C.POINTER(C.c_char_p)),
        ("attribute_types", C.POINTER(C.c_int)),
        ("all_records", C.POINTER(C.POINTER(Record))),
        ("num_records", C.c_int),
        ("datafile", C.c_char_p),
        ("record_block", C.c_void_p),
    ]


# ---- include/pqps_hip.h -------------------------------------------------------
class Column(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_uint32), ("reserved", C.c_uint32)]


class Leaf(C.Structure):
    _fields_ = [("column", C.c_uint32), ("negate", C.c_uint32), ("lo", C.c_uint64), ("span", C.c_uint64)]


class Predicate(C.Structure):
    _fields_ = [
        ("n_leaves", C.c_uint32),
        ("n_columns", C.c_uint32),
        ("truth", C.c_uint64),
        ("leaf", Leaf * MAX_LEAVES),
        ("on_true", C.c_uint8 * MAX_LEAVES),
        ("on_false", C.c_uint8 * MAX_LEAVES),
        ("order", C.c_uint8 * MAX_LEAVES),
    ]


class Pass(C.Structure):
    """struct hipPass (include/hipPredicate.h)."""
    _fields_ = [("pred", Predicate), ("column_ids", C.c_int * MAX_COLUMNS),
                ("member", C.c_int), ("member_column", C.c_int), ("member_form", C.c_int), ("member_base", C.c_uint32),
                ("member_bits", C.c_uint64), ("member_bitmap", C.POINTER(C.c_uint32)), ("member_list", C.POINTER(C.c_uint64)),
                ("member_count", C.c_uint32), ("member_set", C.c_uint32)]


class Plan(C.Structure):
    _fields_ = [("n_passes", C.c_int), ("passes", C.POINTER(Pass))]


class AssignTarget(C.Structure):
    """pqps_assign_target (include/pqps_hip.h)."""
    _fields_ = [("data", C.c_void_p), ("width", C.c_uint32), ("value", C.c_uint64)]


COUNT_MANY_MAX = 16                                          # PQPS_COUNT_MANY_MAX
COUNT_CONSTANT, COUNT_ALONE = -1, -2                         # HIPCOUNT_* (include/hipPredicate.h)


class CountQuery(C.Structure):
    """pqps_count_query (include/pqps_hip.h)."""
    _fields_ = [("n_steps", C.c_uint32), ("leaf", C.c_uint8 * TT_LEAVES), ("on_true", C.c_uint8 * TT_LEAVES),
                ("on_false", C.c_uint8 * TT_LEAVES), ("constant", C.c_uint8)]


class CountMany(C.Structure):
    """pqps_count_many (include/pqps_hip.h)."""
    _fields_ = [("n_queries", C.c_uint32), ("n_leaves", C.c_uint32), ("n_columns", C.c_uint32),
                ("leaf", Leaf * MAX_LEAVES), ("query", CountQuery * COUNT_MANY_MAX)]


class CountPackQuery(C.Structure):                           # struct hipCountQuery
    _fields_ = [("pred", C.POINTER(Predicate)), ("column_ids", C.POINTER(C.c_int))]


class CountBatch(C.Structure):                               # struct hipCountBatch
    _fields_ = [("prog", CountMany), ("column_ids", C.c_int * MAX_COLUMNS)]


class CountPlace(C.Structure):                               # struct hipCountPlace
    _fields_ = [("batch", C.c_int), ("position", C.c_int), ("constant", C.c_int)]


assert C.sizeof(CountQuery) == 24 and C.sizeof(CountMany) == 16 + 24 * MAX_LEAVES + 24 * COUNT_MANY_MAX


class SynthCols(C.Structure):
    _fields_ = [
        ("command_id", C.c_void_p), ("exit_code", C.c_void_p), ("user_id", C.c_void_p),
        ("risk_level", C.c_void_p), ("sudo_used", C.c_void_p), ("shell_code", C.c_void_p),
        ("user_code", C.c_void_p), ("host_code", C.c_void_p), ("base_code", C.c_void_p),
    ]


# ---- include/hipPredicate.h ----------------------------------------------------
class ColumnInfo(C.Structure):
    _fields_ = [("present", C.c_int), ("kind", C.c_int), ("width", C.c_uint32),
                ("dict_count", C.c_int), ("dict", C.POINTER(C.c_char_p))]


class Schema(C.Structure):
    _fields_ = [("col", ColumnInfo * MAX_COLUMNS)]


class Assignment(C.Structure):
    """struct hipAssignment (include/hipPredicate.h)."""
    _fields_ = [("column", C.c_int), ("kind", C.c_int), ("value", C.c_uint64), ("present", C.c_int), ("rank", C.c_uint32),
                ("text", C.c_char_p)]


assert C.sizeof(Record) == 1040 and C.sizeof(WhereClause) == 56
assert C.sizeof(Predicate) == 880 and C.sizeof(Pass) == 976          # struct hipPass: a smaller mirror would be overwritten
assert C.sizeof(ResultSet) == 48 and C.sizeof(EngineS) == 72


class OrderField(C.Structure):                               # pqps_order_field
    _fields_ = [("col", Column), ("base", C.c_uint32), ("bits", C.c_uint32), ("shift", C.c_uint32), ("descending", C.c_int)]


class OrderKey(C.Structure):                                 # struct hipOrderKey
    _fields_ = [("column", C.c_char_p), ("descending", C.c_bool)]


class OrderPlanField(C.Structure):                           # struct hipOrderField
    _fields_ = [("column", C.c_int), ("kind", C.c_int), ("descending", C.c_int),
                ("base", C.c_uint32), ("bits", C.c_uint32), ("shift", C.c_uint32)]


ORDER_MAX_KEYS = 4                                           # HIP_ORDER_MAX_KEYS
ORDER_ROWS, ORDER_ONE, ORDER_PACK32, ORDER_PACK64, ORDER_CHAIN = range(5)   # HIPORDER_*


class OrderKeyPlan(C.Structure):                             # struct hipOrderKeyPlan
    _fields_ = [("form", C.c_int), ("n_fields", C.c_int), ("total_bits", C.c_uint32), ("field", OrderPlanField * ORDER_MAX_KEYS)]


class PqpsError(RuntimeError):
    pass


# ---- WHERE lists ------------------------------------------------------------------
# A python "chain" alternates items and "AND"/"OR"; an item is (attr, op, value[, value_type])
# or a nested chain (list):
#   [("sudo_used","=","TRUE"), "OR", [("risk_level","=","5"), "AND", ("shell_type","=","bash")]]
class WhereList:
    """Owns the ctypes nodes of one whereClauseS list."""

    def __init__(self, chain):
        self._keep = []
        self.head = self._build(chain)

    def _build(self, chain):
        if not chain:
            return None
        items, ops = chain[0::2], chain[1::2]
        nodes = []
        for it in items:
            n = WhereClause()
            if isinstance(it, list):
                sub = self._build(it)
                n.sub = C.pointer(sub) if sub is not None else None
            else:
                a, o, v = it[:3]
                n.attribute = a.encode() if a is not None else None
                n.operator = o.encode() if o is not None else None
                n.value = v.encode("latin-1") if v is not None else None
                n.value_type = it[3] if len(it) > 3 else 0
            self._keep.append(n)
            nodes.append(n)
        for i, n in enumerate(nodes[:-1]):
            n.next = C.pointer(nodes[i + 1])
            n.logical_op = ops[i].encode() if ops[i] is not None else None
        return nodes[0]

    @property
    def ptr(self):
        return C.byref(self.head) if self.head is not None else None


def in_list(values) -> str:
    """The value text of `IN` / `NOT IN` for `values` (str, bytes as latin-1, int or bool): every item single-quoted,
    a quote inside it doubled -- ("a", "it's") -> "('a', 'it''s')"."""
    def text(v):
        if isinstance(v, bytes):
            v = v.decode("latin-1")
        elif isinstance(v, bool):
            v = "true" if v else "false"
        return "'" + str(v).replace("'", "''") + "'"
    return "(" + ", ".join(text(v) for v in values) + ")"


def like_escape(text: str) -> str:
    """`text` as a LIKE pattern that matches itself: `%`, `_` and the backslash escaped."""
    return text.replace("\\", "\\\\").replace("%", "\\%").replace("_", "\\_")


# ---- library --------------------------------------------------------------------------
_lib = None


def build_library():
    """`make` in the package directory (hipcc --offload-arch=gfx950 + gcc)."""
    subprocess.run(["make", "-s", "-C", str(PKG_DIR)], check=True)


_bench_lib = None


def bench_lib():
    """libpqps_bench.so: the lab bench above the engine API (host/engineBench.c) -- not part of the product library."""
    global _bench_lib
    if _bench_lib is None:
        lib()                                                    # the product first: the bench library links against it
        path = PKG_DIR / "libpqps_bench.so"
        if not path.exists():
            raise PqpsError(f"{path} is missing: build it with `make -C {PKG_DIR}`")
        B = C.CDLL(str(path))
        B.hipEngineBench.argtypes = [C.POINTER(C.POINTER(EngineS)), C.c_int, C.POINTER(WhereClause), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(BenchResult)]
        _bench_lib = B
    return _bench_lib


def lib():
    """The product shared object.  Never falls back to anything else."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise PqpsError(f"{LIB_PATH} is missing: build it with `make -C {PKG_DIR}` "
                        "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(str(LIB_PATH))
    W = C.POINTER(WhereClause)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.pqps_last_error.restype = C.c_char_p
    L.pqps_last_kernel.restype = C.c_char_p
    L.pqps_ctx_device.argtypes = [vp]
    L.pqps_copy_peer.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
    L.pqps_device_count.restype = C.c_int
    L.pqps_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.pqps_ctx_destroy.argtypes = [vp]
    L.pqps_ctx_destroy.restype = None
    L.pqps_ctx_sync.argtypes = [vp, vp]
    L.pqps_ctx_reserve.argtypes = [vp, u64]
    L.pqps_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_long]
    L.pqps_ctx_set_timing.argtypes = [vp, C.c_int]
    L.pqps_ctx_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.pqps_device_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int), C.POINTER(u64)]
    L.pqps_malloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.pqps_free.argtypes = [vp, vp]
    L.pqps_memset.argtypes = [vp, vp, C.c_int, C.c_size_t, vp]
    L.pqps_upload.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.pqps_download.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.pqps_filter_scan.argtypes = [vp, C.POINTER(Column), u32, u64, u32, C.POINTER(Predicate), vp, u64, vp, vp]
    L.pqps_filter_count.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), vp, vp]
    L.pqps_filter_count_many.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(CountMany), vp, vp]
    L.pqps_filter_flags.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), vp, vp, vp]
    L.pqps_filter_gather.argtypes = [vp, C.POINTER(Column), u32, vp, vp, u64, u32, C.POINTER(Predicate), vp, u64, vp, vp]
    L.pqps_index_build.argtypes = [vp, C.POINTER(Column), u64, C.c_int, vp, vp, vp]
    L.pqps_index_probe.argtypes = [vp, vp, u32, C.c_int, u64, u64, u64, vp, vp]
    L.pqps_index_select.argtypes = [vp, C.POINTER(Column), u32, C.POINTER(Column), vp, vp, C.c_int, u64, u64, u64, u32, C.POINTER(Predicate), vp, vp, u64, vp, vp]
    L.pqps_partition.argtypes = [u64, C.c_int, C.c_int, C.POINTER(u64), C.POINTER(u64)]
    L.pqps_partition.restype = None
    L.pqps_synth_user_tables.argtypes = [u64, vp, vp]
    L.pqps_synth_user_tables.restype = None
    L.pqps_synth_generate.argtypes = [vp, u64, u64, u64, vp, vp, C.POINTER(SynthCols), vp]
    L.pqps_synth_generate_host.argtypes = [u64, u64, u64, vp, vp, C.POINTER(SynthCols)]
    L.pqps_synth_generate_host.restype = None
    L.pqps_bump_codes.argtypes = [vp, vp, u32, u64, u32, vp]
    L.pqps_pack_bits.argtypes = [vp, vp, u64, vp, u64, u64, vp]
    L.pqps_pack12.argtypes = [vp, vp, u64, vp, u64, u64, vp]
    L.pqps_member_flags.argtypes = [vp, C.POINTER(Column), u64, C.c_int, u32, u64, vp, vp, u32, C.c_int, vp, vp, vp]
    L.hipIsSetOperator.argtypes = [C.c_char_p]
    L.pqps_filter_assign.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(AssignTarget), u32, vp, vp]
    L.pqps_assign_flags.argtypes = [vp, vp, u64, C.POINTER(AssignTarget), u32, vp]
    L.hipCompileAssignments.argtypes = [C.POINTER(Schema), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int, C.POINTER(Assignment)]
    L.pqps_compact_rows.argtypes = [vp, C.POINTER(Column), u32, u64, vp, C.POINTER(u64), vp]
    L.pqps_project_column.argtypes = [vp, C.POINTER(Column), vp, vp, u64, u32, vp, vp]
    L.pqps_gather_keys.argtypes = [vp, C.POINTER(Column), C.c_int, vp, vp, u64, u32, vp, vp]
    L.pqps_merge_index_slots.argtypes = [vp, vp, vp, u32, u64, vp, u64, vp, vp]
    L.pqps_merge_slots.argtypes = [vp, vp, u32, u64, vp, u64, vp, vp]
    L.pqps_qstream_create.argtypes = [vp, u32, C.POINTER(vp)]
    L.pqps_qstream_scan.argtypes = [vp, C.POINTER(Column), u32, u64, u32, C.POINTER(Predicate), vp, u64, vp, vp]
    L.pqps_qstream_count.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), vp, vp]
    L.pqps_qstream_sync.argtypes = [vp]
    L.pqps_qstream_hint_answer.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.pqps_qstream_hint_answer.restype = None
    L.pqps_qstream_scan_slot.argtypes = [vp, u32, C.POINTER(Column), u32, u64, u32, C.POINTER(Predicate), vp, u64, vp, vp]
    L.pqps_qstream_count_slot.argtypes = [vp, u32, C.POINTER(Column), u32, u64, C.POINTER(Predicate), vp, vp]
    L.pqps_qstream_wait.argtypes = [vp, u32]
    L.pqps_qstream_lane.argtypes = [vp, u32, u64, vp, C.POINTER(vp), C.POINTER(vp)]
    L.pqps_qstream_mark.argtypes = [vp, u32]
    L.pqps_qstream_set_timing.argtypes = [vp, C.c_int]
    L.pqps_qstream_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.pqps_qstream_wait_ns.argtypes = [vp, C.c_int]
    L.pqps_qstream_wait_ns.restype = u64
    L.pqps_exchange_wait_ns.argtypes = [vp, C.c_int]
    L.pqps_exchange_wait_ns.restype = u64
    L.pqps_qstream_destroy.argtypes = [vp]
    L.pqps_exchange_unique_id.argtypes = [C.c_char_p, vp]
    L.pqps_exchange_create.argtypes = [vp, C.c_char_p, vp, u32, u32, u64, u32, C.POINTER(vp)]
    L.pqps_exchange_prepare.argtypes = [vp, C.c_char_p, u32, u32, u64, u32, C.POINTER(vp)]
    L.pqps_exchange_connect.argtypes = [vp, vp]
    L.pqps_exchange_select.argtypes = [vp, C.POINTER(Column), u32, u64, u32, C.POINTER(Predicate), u32, vp]
    L.pqps_exchange_count.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), u32, vp]
    L.pqps_exchange_result.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.pqps_exchange_sync.argtypes = [vp]
    L.pqps_exchange_wire_bytes.argtypes = [vp, C.POINTER(u64), C.c_int]
    L.pqps_wire_bytes.argtypes = [u64, u64]
    L.pqps_wire_bytes.restype = u64
    L.pqps_wire_pays.argtypes = [u64, u64]
    L.pqps_wire_pack.argtypes = [vp, vp, u64, u64, u32, C.c_int, vp, vp, vp]
    L.pqps_wire_expand.argtypes = [vp, vp, u64, u32, vp, vp]
    L.pqps_exchange_wire_bytes.restype = None
    L.pqps_exchange_eager.argtypes = [vp, C.POINTER(u64), C.c_int]
    L.pqps_exchange_eager.restype = None
    L.pqps_exchange_destroy.argtypes = [vp]
    L.hipCompileWhere.argtypes = [C.POINTER(Schema), W, C.POINTER(Predicate), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.hipCompileWherePlan.argtypes = [C.POINTER(Schema), W, C.POINTER(Plan), C.c_char_p, C.c_size_t]
    L.hipCompileWherePlanSets.argtypes = [C.POINTER(Schema), W, C.POINTER(SetInfo), C.c_int, C.POINTER(Plan), C.c_char_p, C.c_size_t]
    L.hipCompileHaving.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.POINTER(Having)]
    L.pqps_bins_having.argtypes = [vp, vp, u32, C.c_int, C.c_int, C.c_int, u64, C.c_int, vp, vp, vp]
    L.pqps_bins_rows.argtypes = [vp, vp, u32, C.c_int, vp, vp]
    L.hipPlanFree.argtypes = [C.POINTER(Plan)]
    L.hipPlanFree.restype = None
    L.hipColumnId.argtypes = [C.c_char_p]
    for name in ("hipDumpTokens", "hipDumpParse"):
        f = getattr(L, name)
        f.restype = C.c_longlong
        f.argtypes = [C.c_char_p, C.c_char_p, C.c_longlong]
    # engine API (include/executeEngine-hip.h)
    E = C.POINTER(EngineS)
    L.initializeEngineHIP.restype = E
    L.initializeEngineHIP.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_char_p, C.c_char_p]
    L.initializeEngineSyntheticHIP.restype = E
    L.initializeEngineSyntheticHIP.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_char_p]
    L.initializeEngineColumnsHIP.restype = E
    L.initializeEngineColumnsHIP.argtypes = [C.c_ulonglong, C.POINTER(ColumnData), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_char_p]
    L.hipSyntheticDictionary.restype = C.POINTER(C.c_char_p)
    L.hipSyntheticDictionary.argtypes = [C.c_int, C.POINTER(C.c_int)]
    for name in ("executeQuerySelectAsyncHIP", "executeQueryCountAsyncHIP"):
        f = getattr(L, name)
        f.restype = vp
        f.argtypes = [E, W]
    L.awaitQueryHIP.restype = C.c_longlong
    L.awaitQueryHIP.argtypes = [vp, C.POINTER(DeviceResult)]
    L.releaseQueryHIP.argtypes = [vp]
    L.releaseQueryHIP.restype = None
    L.hipEngineLanes.argtypes = [E]
    L.initializeEngineSyntheticRankHIP.restype = E
    L.initializeEngineSyntheticRankHIP.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_int, C.c_char_p]
    L.hipEngineRcclIdHIP.argtypes = [C.c_char_p, vp]
    L.hipEngineJoinRanksHIP.argtypes = [E, C.c_char_p, vp]
    L.hipEngineJoinPrepareHIP.argtypes = [E, C.c_char_p]
    L.hipEngineJoinConnectHIP.argtypes = [E, vp]
    L.hipEngineLeaveRanksHIP.argtypes = [E]
    L.hipEngineWireBytesHIP.argtypes = [E, C.POINTER(C.c_ulonglong), C.c_int]
    L.hipEngineEagerQueriesHIP.argtypes = [E, C.POINTER(C.c_ulonglong), C.c_int]
    L.hipQueryChecksumHIP.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    L.pqps_ids_checksum.argtypes = [vp, vp, u64, C.POINTER(u64), vp]
    L.pqps_qstream_reserve.argtypes = [vp, u64]
    L.pqps_qstream_test_fail_slot.argtypes = [vp, u32]
    L.hipEngineProbeBoolIndexes.argtypes = [E, C.c_int]
    L.hipEngineKernelTiming.argtypes = [E, C.c_int]
    L.hipEngineKernelTime.argtypes = [E, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.pqps_malloc_mapped.argtypes = [vp, C.c_size_t, C.POINTER(vp), C.POINTER(vp)]
    L.pqps_free_mapped.argtypes = [vp, vp]
    L.destroyEngineHIP.argtypes = [E]
    L.destroyEngineHIP.restype = None
    L.executeQuerySelectHIP.restype = C.POINTER(ResultSet)
    L.executeQuerySelectHIP.argtypes = [E, C.POINTER(C.c_char_p), C.c_int, C.c_char_p, W]
    L.executeQuerySelectIdsHIP.restype = C.c_longlong
    L.executeQuerySelectIdsHIP.argtypes = [E, W, C.POINTER(C.POINTER(C.c_uint)), C.POINTER(C.c_double)]
    L.hipEngineShards.restype = C.c_int
    L.hipEngineShards.argtypes = [E, C.POINTER(C.c_ulonglong), C.c_int]
    L.executeQueryCountHIP.restype = C.c_longlong
    L.executeQueryCountHIP.argtypes = [E, W]
    L.executeQueryCountManyHIP.restype = C.c_longlong
    L.executeQueryCountManyHIP.argtypes = [E, C.POINTER(W), C.c_int, C.POINTER(C.c_longlong)]
    L.hipCountManyPack.argtypes = [C.POINTER(CountPackQuery), C.c_int, C.c_int, C.POINTER(CountBatch), C.POINTER(C.c_int),
                                   C.POINTER(CountPlace)]
    L.executeQueryGroupCountHIP.restype = C.POINTER(GroupResult)
    L.executeQueryGroupCountHIP.argtypes = [E, C.c_char_p, W]
    L.freeGroupResultHIP.argtypes = [C.POINTER(GroupResult)]
    L.freeGroupResultHIP.restype = None
    L.pqps_filter_group.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(Column), u32, u32, vp, vp]
    L.pqps_group_list.argtypes = [vp, C.POINTER(Column), u64, vp, vp, u64, u32, u32, u32, vp, vp]
    L.pqps_column_bounds.argtypes = [vp, C.POINTER(Column), u64, vp, vp]
    L.executeQueryAggregateHIP.restype = C.POINTER(AggregateResult)
    L.executeQueryAggregateHIP.argtypes = [E, C.c_char_p, C.c_char_p, W]
    L.freeAggregateResultHIP.argtypes = [C.POINTER(AggregateResult)]
    L.freeAggregateResultHIP.restype = None
    L.pqps_filter_aggregate.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(Column), C.POINTER(Column),
                                        u32, u32, vp, vp]
    L.pqps_aggregate_list.argtypes = [vp, C.POINTER(Column), C.POINTER(Column), u64, vp, vp, u64, u32, u32, u32, vp, vp]
    L.executeQueryGroupBucketsHIP.restype = C.POINTER(BucketResult)
    L.executeQueryGroupBucketsHIP.argtypes = [E, C.c_char_p, C.c_int, C.c_longlong, C.c_char_p, W]
    L.freeBucketResultHIP.argtypes = [C.POINTER(BucketResult)]
    L.freeBucketResultHIP.restype = None
    L.pqps_filter_group_buckets.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(Column), u32, vp, u32, u32, vp, vp]
    L.pqps_group_buckets_list.argtypes = [vp, C.POINTER(Column), u64, vp, vp, u64, u32, u32, vp, u32, u32, vp, vp]
    L.pqps_filter_aggregate_buckets.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(Column), C.POINTER(Column),
                                                u32, vp, u32, u32, vp, vp]
    L.pqps_aggregate_buckets_list.argtypes = [vp, C.POINTER(Column), C.POINTER(Column), u64, vp, vp, u64, u32, u32, vp, u32, u32, vp, vp]
    L.hipBucketBounds.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                  C.POINTER(C.POINTER(u32)), C.POINTER(C.POINTER(C.c_longlong)), C.POINTER(u32)]
    L.executeQueryGroupPairHIP.restype = C.POINTER(GroupPairResult)
    L.executeQueryGroupPairHIP.argtypes = [E, C.c_char_p, C.c_char_p, C.c_char_p, W]
    L.freeGroupPairResultHIP.argtypes = [C.POINTER(GroupPairResult)]
    L.freeGroupPairResultHIP.restype = None
    L.pqps_filter_group_pair.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(Column), u32, u32,
                                         C.POINTER(Column), u32, u32, C.POINTER(Column), vp, vp]
    L.pqps_group_pair_list.argtypes = [vp, C.POINTER(Column), u32, u32, C.POINTER(Column), u32, u32, C.POINTER(Column), u64, vp, vp,
                                       u64, u32, vp, vp]
    L.pqps_group_pair_sort.argtypes = [vp, C.POINTER(Column), u32, u32, C.POINTER(Column), u32, u32, C.POINTER(Column), u64, vp, u64,
                                       u32, C.POINTER(vp), C.POINTER(u64), vp]
    L.executeQueryGroupTopHIP.restype = C.POINTER(GroupTopResult)
    L.executeQueryGroupTopHIP.argtypes = [E, C.c_char_p, C.c_char_p, C.c_int, C.c_bool, C.c_longlong, W]
    L.freeGroupTopResultHIP.argtypes = [C.POINTER(GroupTopResult)]
    L.freeGroupTopResultHIP.restype = None
    L.pqps_filter_group_wide.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(Column), C.POINTER(Column),
                                         u32, u32, vp, vp]
    L.pqps_group_wide_list.argtypes = [vp, C.POINTER(Column), C.POINTER(Column), u64, vp, vp, u64, u32, u32, u32, vp, vp]
    L.pqps_bins_compact.argtypes = [vp, vp, u32, C.c_int, C.POINTER(vp), C.POINTER(u64), vp]
    L.pqps_group_sort.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Column), u64, vp, u64, u32, C.POINTER(vp), C.POINTER(u64), vp]
    L.hipGroupTopOrder.restype = C.c_longlong
    L.hipGroupTopOrder.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, C.c_int, C.c_int, C.c_longlong, vp]
    L.hipEngineCreateSetHIP.restype = C.POINTER(ValueSetResult)
    L.hipEngineCreateSetHIP.argtypes = [E, C.c_char_p, W, C.POINTER(SetHaving)]
    L.hipEngineSetKeysHIP.restype = C.POINTER(SetKeysResult)
    L.hipEngineSetKeysHIP.argtypes = [E, C.POINTER(ValueSetResult)]
    L.freeSetKeysHIP.argtypes = [C.POINTER(SetKeysResult)]
    L.freeSetKeysHIP.restype = None
    L.hipEngineFreeSetHIP.argtypes = [E, C.POINTER(ValueSetResult)]
    L.executeQueryCountDistinctHIP.restype = C.POINTER(DistinctResult)
    L.executeQueryCountDistinctHIP.argtypes = [E, C.c_char_p, C.c_char_p, W]
    L.freeDistinctResultHIP.argtypes = [C.POINTER(DistinctResult)]
    L.freeDistinctResultHIP.restype = None
    L.pqps_distinct_bitmap_words.restype = u64
    L.pqps_distinct_bitmap_words.argtypes = [u32, u32]
    L.pqps_filter_distinct.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(Column), u32, u32,
                                       C.POINTER(Column), u32, u32, vp, vp, vp, vp]
    L.pqps_distinct_list.argtypes = [vp, C.POINTER(Column), u32, u32, C.POINTER(Column), u32, u32, u64, vp, vp, u64, u32, vp, vp, vp]
    L.pqps_distinct_count.argtypes = [vp, vp, u32, u32, vp, vp]
    L.pqps_distinct_sort.argtypes = [vp, C.POINTER(Column), u32, C.POINTER(Column), u32, u32, vp, u64, u32, vp, vp, vp]
    L.executeQueryOrderIdsHIP.restype = C.c_longlong
    L.executeQueryOrderIdsHIP.argtypes = [E, W, C.c_char_p, C.c_bool, C.c_longlong, C.POINTER(C.POINTER(C.c_uint)),
                                          C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    L.pqps_topk_scratch_bytes.restype = u64
    L.pqps_topk_scratch_bytes.argtypes = [vp, u64, u32, C.c_int, C.c_int]
    L.pqps_filter_topk.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(Column), C.c_int, C.c_int, u32, u32,
                                   vp, u64, vp, vp, vp]
    L.pqps_topk_list.argtypes = [vp, C.POINTER(Column), C.c_int, C.c_int, vp, u64, u32, u32, vp, u64, vp, vp]
    L.pqps_sort_list.argtypes = [vp, C.POINTER(Column), C.c_int, C.c_int, vp, u64, u32, vp, vp, vp]
    L.pqps_filter_topk_multi.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(OrderField), u32, u32, u32,
                                         vp, u64, vp, vp, vp]
    L.pqps_topk_list_multi.argtypes = [vp, C.POINTER(OrderField), u32, vp, u64, u32, u32, vp, u64, vp, vp]
    L.pqps_sort_list_multi.argtypes = [vp, C.POINTER(OrderField), u32, vp, u64, u32, vp, vp, vp]
    L.pqps_sort_list_chain.argtypes = [vp, C.POINTER(Column), C.POINTER(C.c_int), C.POINTER(C.c_int), u32, vp, u64, u32, vp, vp, vp]
    L.hipOrderKeyPlan.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.POINTER(C.c_int), C.POINTER(OrderKeyPlan)]
    L.executeQueryOrderIdsByHIP.restype = C.c_longlong
    L.executeQueryOrderIdsByHIP.argtypes = [E, W, C.POINTER(OrderKey), C.c_int, C.c_longlong, C.POINTER(C.POINTER(C.c_uint)),
                                            C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    L.pqps_filter_group_first.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(Column), C.c_int, C.c_int, u32,
                                          C.POINTER(Column), u32, u32, vp, vp, vp, vp]
    L.pqps_group_first_list.argtypes = [vp, C.POINTER(Column), C.c_int, C.c_int, C.POINTER(Column), u32, u32, u64, vp, vp, u64, u32,
                                        vp, vp, vp]
    L.hipFirstKeyDecode.argtypes = [C.c_int, C.c_int, C.c_ulonglong, C.POINTER(C.c_longlong), C.POINTER(C.c_uint)]
    L.executeQueryGroupFirstHIP.restype = C.POINTER(GroupFirstResult)
    L.executeQueryGroupFirstHIP.argtypes = [E, C.c_char_p, C.c_char_p, C.c_bool, W]
    L.freeGroupFirstResultHIP.argtypes = [C.POINTER(GroupFirstResult)]
    L.freeGroupFirstResultHIP.restype = None
    L.pqps_filter_group_head.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(Column), C.c_int, C.c_int, u32,
                                         C.POINTER(Column), u32, u32, u32, vp, vp, vp, vp]
    L.pqps_group_head_list.argtypes = [vp, C.POINTER(Column), C.c_int, C.c_int, C.POINTER(Column), u32, u32, u64, vp, vp, u64, u32,
                                       u32, vp, vp, vp]
    L.pqps_runs_head_flags.argtypes = [vp, vp, u64, u64, vp, vp]
    L.pqps_group_head_sort.argtypes = [vp, C.POINTER(Column), C.c_int, C.c_int, C.POINTER(Column), C.c_int, vp, u64, u32, u64, C.c_int,
                                       vp, vp, C.POINTER(u64), vp]
    L.hipHeadMerge.restype = C.c_longlong
    L.hipHeadMerge.argtypes = [C.POINTER(HeadList), C.c_int, C.c_longlong, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                               C.POINTER(C.c_uint64)]
    L.pqps_filter_digit_hist.argtypes = [vp, C.POINTER(Column), u32, u64, C.POINTER(Predicate), C.POINTER(Column), C.c_int, u64, u32,
                                         C.POINTER(Column), u32, u32, u32, vp, u32, u32, vp, vp]
    L.pqps_digit_hist_list.argtypes = [vp, C.POINTER(Column), C.c_int, u64, u32, C.POINTER(Column), u32, u32, u32, vp, u32, u32, u64,
                                       vp, vp, u64, u32, vp, vp]
    L.hipQuantileRank.restype = C.c_ulonglong
    L.hipQuantileRank.argtypes = [C.c_ulonglong, C.c_uint]
    L.hipQuantileDigitBits.restype = C.c_uint
    L.hipQuantileDigitBits.argtypes = [C.c_uint, C.c_uint, C.c_ulonglong]
    L.hipQuantilePick.argtypes = [C.POINTER(C.c_uint64), C.c_uint, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.executeQueryQuantilesHIP.restype = C.POINTER(QuantileResult)
    L.executeQueryQuantilesHIP.argtypes = [E, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint), C.c_int, W]
    L.freeQuantileResultHIP.argtypes = [C.POINTER(QuantileResult)]
    L.freeQuantileResultHIP.restype = None
    L.executeQueryGroupHeadHIP.restype = C.POINTER(GroupHeadResult)
    L.executeQueryGroupHeadHIP.argtypes = [E, C.c_char_p, C.c_char_p, C.c_bool, C.c_longlong, W]
    L.freeGroupHeadResultHIP.argtypes = [C.POINTER(GroupHeadResult)]
    L.freeGroupHeadResultHIP.restype = None
    CR = C.POINTER(ColumnarResult)
    L.executeQuerySelectGroupHeadHIP.restype = CR
    L.executeQuerySelectGroupHeadHIP.argtypes = [E, C.POINTER(C.c_char_p), C.c_int, W, C.c_char_p, C.c_char_p, C.c_bool, C.c_longlong,
                                                 C.POINTER(C.c_longlong), C.POINTER(C.POINTER(C.c_longlong))]
    L.executeQuerySelectColumnarHIP.restype = CR
    L.executeQuerySelectColumnarHIP.argtypes = [E, C.POINTER(C.c_char_p), C.c_int, W]
    L.executeQuerySelectOrderedHIP.restype = CR
    L.executeQuerySelectOrderedHIP.argtypes = [E, C.POINTER(C.c_char_p), C.c_int, W, C.c_char_p, C.c_bool, C.c_longlong,
                                               C.POINTER(C.c_longlong)]
    L.executeQuerySelectGroupFirstHIP.restype = CR
    L.executeQuerySelectGroupFirstHIP.argtypes = [E, C.POINTER(C.c_char_p), C.c_int, W, C.c_char_p, C.c_char_p, C.c_bool,
                                                  C.POINTER(C.c_longlong)]
    L.executeQuerySelectOrderedByHIP.restype = CR
    L.executeQuerySelectOrderedByHIP.argtypes = [E, C.POINTER(C.c_char_p), C.c_int, W, C.POINTER(OrderKey), C.c_int, C.c_longlong,
                                                 C.POINTER(C.c_longlong)]
    L.freeColumnarResultHIP.argtypes = [CR]
    L.hipColumnarCellText.restype = vp
    L.hipColumnarCellText.argtypes = [CR, C.c_int, C.c_int]
    L.hipColumnarHead.restype = C.POINTER(ResultSet)
    L.hipColumnarHead.argtypes = [CR, C.c_int]
    L.freeResultSetHead.argtypes = [C.POINTER(ResultSet), C.c_int]
    L.executeQueryDeleteHIP.restype = C.POINTER(ResultSet)
    L.executeQueryDeleteHIP.argtypes = [E, C.c_char_p, W]
    L.executeQueryUpdateHIP.restype = C.c_longlong
    L.executeQueryUpdateHIP.argtypes = [E, C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int, W, C.POINTER(C.c_double)]
    L.executeQueryInsertColumnsHIP.restype = C.c_longlong
    L.executeQueryInsertColumnsHIP.argtypes = [E, C.c_char_p, C.c_ulonglong, C.POINTER(ColumnData), C.POINTER(C.c_double)]
    L.executeQueryInsertRowsHIP.restype = C.c_longlong
    L.executeQueryInsertRowsHIP.argtypes = [E, C.c_char_p, C.POINTER(Record), C.c_ulonglong, C.POINTER(C.c_double)]
    L.hipMergeDictionaries.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(C.c_char_p),
                                       C.POINTER(C.c_int), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_int)]
    L.pqps_remap_codes.argtypes = [vp, vp, u32, vp, u32, u64, vp, u32, C.c_int, vp, vp]
    L.pqps_remap_form.argtypes = [u32]
    L.executeQueryInsertHIP.restype = C.c_bool
    L.executeQueryInsertHIP.argtypes = [E, C.c_char_p, C.POINTER(Record)]
    L.addAttributeIndexHIP.restype = C.c_bool
    L.addAttributeIndexHIP.argtypes = [E, C.c_char_p, C.c_char_p, C.c_int]
    L.freeResultSet.argtypes = [C.POINTER(ResultSet)]
    L.freeResultSet.restype = None
    L.evaluateWhereClause.restype = C.c_bool
    L.evaluateWhereClause.argtypes = [C.POINTER(Record), W]
    L.linearSearchRecords.restype = C.POINTER(C.POINTER(Record))
    L.linearSearchRecords.argtypes = [C.POINTER(C.POINTER(Record)), C.c_int, W, C.POINTER(C.c_int)]
    L.isAttributeIndexed.argtypes = [E, C.c_char_p]
    L.printTable.argtypes = [vp, C.POINTER(ResultSet), C.c_int]
    L.printTable.restype = None
    L.run_test_query.argtypes = [E, C.c_char_p, C.c_int]
    L.run_test_query.restype = None
    L.free.argtypes = [vp]
    L.free.restype = None
    _lib = L
    return L


def check(rc, what="pqps call"):
    if rc != 0:
        raise PqpsError(f"{what} failed ({rc}): {lib().pqps_last_error().decode()}")


# ---- predicate compile --------------------------------------------------------------------
class SchemaSpec:
    """Python-side description of which columns exist (width, dictionary)."""

    def __init__(self):
        self.schema = Schema()
        self._keep = []
        for i, kind in enumerate(COLUMN_KIND):
            self.schema.col[i].kind = kind

    def set_numeric(self, name, width):
        c = self.schema.col[COL[name]]
        c.present, c.width = 1, width
        return self

    def set_dict(self, name, width, values):
        """values: list of bytes, ascending in strcmp (= bytes) order."""
        arr = (C.c_char_p * max(1, len(values)))()
        for i, v in enumerate(values):
            arr[i] = v
        self._keep.append(arr)
        c = self.schema.col[COL[name]]
        c.present, c.width, c.dict_count, c.dict = 1, width, len(values), arr
        return self


def compile_plan_sets(spec: SchemaSpec, chain, sets=None):
    """-> [(Predicate, [column id per slot], member), ...]: the passes of hipCompileWherePlan.  A column id >= MAX_COLUMNS
    names the flags of pass (id - MAX_COLUMNS); the last pass is the query's result.  `member` is None for a filter pass;
    for a member pass (a LIKE / IN set, include/hipPredicate.h; its Predicate is empty) it is a dict: "column" (id), "form"
    (MEMBER_BITMAP / MEMBER_LIST), "base", "n_bits", "words" (the bitmap's u32 words), "values" (the sorted list) and "set"
    (the id of the value set an IN SET node names, 0 otherwise: such a pass has no words of its own).
    `sets`: the table of value sets the chain may name (hipCompileWherePlanSets) -- dicts with "id", "column" (name or id),
    "kind", "base", "n_bits", "members", "stale"; None compiles through hipCompileWherePlan itself."""
    wl = WhereList(chain)
    plan = Plan()
    err = C.create_string_buffer(200)
    if sets is None:
        rc = lib().hipCompileWherePlan(C.byref(spec.schema), wl.ptr, C.byref(plan), err, 200)
    else:
        infos = (SetInfo * max(1, len(sets)))()
        for i, d in enumerate(sets):
            col = d["column"]
            infos[i] = SetInfo(d["id"], COL[col] if isinstance(col, str) else col, d["kind"], d.get("base", 0) & 0xFFFFFFFF,
                               d["n_bits"], d["members"], int(d.get("stale", 0)))
        rc = lib().hipCompileWherePlanSets(C.byref(spec.schema), wl.ptr, infos, len(sets), C.byref(plan), err, 200)
    if rc != 0:
        raise PqpsError("hipCompileWherePlan: " + err.value.decode())
    out = []
    for k in range(plan.n_passes):
        p = plan.passes[k]
        pred = Predicate()
        C.memmove(C.byref(pred), C.byref(p.pred), C.sizeof(Predicate))
        member = None
        if p.member:
            bitmap = p.member_form == MEMBER_BITMAP
            member = dict(column=p.member_column, form=p.member_form, base=p.member_base, n_bits=p.member_bits, set=p.member_set,
                          words=list(p.member_bitmap[:(p.member_bits + 31) // 32]) if bitmap and not p.member_set else [],
                          values=[] if bitmap else list(p.member_list[:p.member_count]))
        out.append((pred, list(p.column_ids[:pred.n_columns]), member))
    lib().hipPlanFree(C.byref(plan))
    return out


def compile_plan(spec: SchemaSpec, chain):
    """-> [(Predicate, [column id per slot]), ...]: compile_plan_sets without the member descriptions."""
    return [(pred, ids) for pred, ids, _ in compile_plan_sets(spec, chain)]


def compile_where(spec: SchemaSpec, chain):
    """-> (Predicate, [column id per slot]).  Raises PqpsError when not expressible."""
    wl = WhereList(chain)
    pred = Predicate()
    ids = (C.c_int * MAX_COLUMNS)()
    err = C.create_string_buffer(200)
    rc = lib().hipCompileWhere(C.byref(spec.schema), wl.ptr, C.byref(pred), ids, err, 200)
    if rc != 0:
        raise PqpsError("hipCompileWhere: " + err.value.decode())
    return pred, list(ids[:pred.n_columns])


def assignment_texts(assignments):
    """{column: str | bytes | int | bool} -> (ctypes array of column names, of value texts, n): the SET list as
    executeQueryUpdateHIP / hipCompileAssignments take it (bytes as they are, a bool as "true" / "false")."""
    def text(v):
        if isinstance(v, bytes):
            return v
        if isinstance(v, bool):
            return b"true" if v else b"false"
        return str(v).encode("latin-1")
    n = len(assignments)
    names = (C.c_char_p * max(1, n))(*[k.encode() for k in assignments])
    values = (C.c_char_p * max(1, n))(*[text(v) for v in assignments.values()])
    return names, values, n


def compile_assignments(spec: SchemaSpec, assignments):
    """hipCompileAssignments: [(column id, kind, value, present, rank), ...] for {column: value text} -- value = the typed
    value (an i32 as a Python int with its sign, a string column's rank), present / rank as struct hipAssignment has them.
    Raises PqpsError when the SET list is refused (reason on stderr)."""
    names, values, n = assignment_texts(assignments)
    out = (Assignment * MAX_COLUMNS)()
    if lib().hipCompileAssignments(C.byref(spec.schema), names, values, n, out) != 0:
        raise PqpsError("hipCompileAssignments refused the SET list (reason on stderr)")
    res = []
    for a in out[:n]:
        v = int(a.value)
        if a.kind == HIPKIND_I32 and v >= 1 << 31:
            v -= 1 << 32
        res.append((a.column, a.kind, v, bool(a.present), int(a.rank)))
    return res


def assign_targets(triples):
    """[(device_ptr, width, value), ...] -> ctypes array of pqps_assign_target."""
    arr = (AssignTarget * max(1, len(triples)))()
    for i, (p, w, v) in enumerate(triples):
        arr[i].data, arr[i].width, arr[i].value = p, w, v & 0xFFFFFFFFFFFFFFFF
    return arr


def filter_assign(ctx, cols, n_cols, n_rows, pred, triples, matched_dev, stream=None):
    """pqps_filter_assign: the fused filter-and-assign launch; `triples` as assign_targets takes them."""
    check(lib().pqps_filter_assign(ctx.h, cols, n_cols, n_rows, C.byref(pred), assign_targets(triples), len(triples), matched_dev, stream),
          "pqps_filter_assign")


def assign_flags(ctx, flags_dev, n_rows, triples, stream=None):
    """pqps_assign_flags: the same stores by byte flags."""
    check(lib().pqps_assign_flags(ctx.h, flags_dev, n_rows, assign_targets(triples), len(triples), stream), "pqps_assign_flags")


def filter_group_first(ctx, cols, n_cols, n_rows, pred, key_col, key_signed, descending, row_base, group_col, bin_base, n_bins,
                       out_dev, best_dev, count_dev, stream=None):
    """pqps_filter_group_first: the fused filter-and-first-row launch; `pred` a Predicate (or its byref), `key_col` /
    `group_col` a Column or None."""
    ref = lambda c: C.byref(c) if c is not None else None
    check(lib().pqps_filter_group_first(ctx.h, cols, n_cols, n_rows, C.byref(pred) if isinstance(pred, Predicate) else pred,
                                        ref(key_col), int(key_signed), int(descending), row_base, ref(group_col), bin_base, n_bins,
                                        out_dev, best_dev, count_dev, stream), "pqps_filter_group_first")


def group_first_list(ctx, key_col, key_signed, descending, group_col, bin_base, n_bins, n_rows, ids_dev, count_dev, capacity, id_base,
                     out_dev, best_dev, stream=None):
    """pqps_group_first_list: the same words over an ID list."""
    ref = lambda c: C.byref(c) if c is not None else None
    check(lib().pqps_group_first_list(ctx.h, ref(key_col), int(key_signed), int(descending), ref(group_col), bin_base, n_bins, n_rows,
                                      ids_dev, count_dev, capacity, id_base, out_dev, best_dev, stream), "pqps_group_first_list")


def filter_group_head(ctx, cols, n_cols, n_rows, pred, key_col, key_signed, descending, row_base, group_col, bin_base, n_bins,
                      n_rounds, out_dev, best_dev, count_dev, stream=None):
    """pqps_filter_group_head: the rounds of the fused filter-and-first-row launch; out_dev holds [n_rounds][n_bins] words."""
    ref = lambda c: C.byref(c) if c is not None else None
    check(lib().pqps_filter_group_head(ctx.h, cols, n_cols, n_rows, C.byref(pred) if isinstance(pred, Predicate) else pred,
                                       ref(key_col), int(key_signed), int(descending), row_base, ref(group_col), bin_base, n_bins,
                                       n_rounds, out_dev, best_dev, count_dev, stream), "pqps_filter_group_head")


def group_head_list(ctx, key_col, key_signed, descending, group_col, bin_base, n_bins, n_rows, ids_dev, count_dev, capacity, id_base,
                    n_rounds, out_dev, best_dev, stream=None):
    """pqps_group_head_list: the same words over an ID list."""
    ref = lambda c: C.byref(c) if c is not None else None
    check(lib().pqps_group_head_list(ctx.h, ref(key_col), int(key_signed), int(descending), ref(group_col), bin_base, n_bins, n_rows,
                                     ids_dev, count_dev, capacity, id_base, n_rounds, out_dev, best_dev, stream), "pqps_group_head_list")


def runs_head_flags(ctx, sorted_keys_dev, n, limit, keep_dev, stream=None):
    """pqps_runs_head_flags: keep[i] = i < limit or sorted_keys[i - limit] != sorted_keys[i]."""
    check(lib().pqps_runs_head_flags(ctx.h, sorted_keys_dev, n, limit, keep_dev, stream), "pqps_runs_head_flags")


def group_head_sort(ctx, key_col, key_signed, descending, group_col, group_signed, ids_dev, n, id_base, limit, repeats, out_ids_dev,
                    out_keys_dev, stream=None):
    """pqps_group_head_sort: the sort form over an ID list; returns the kept entries' count."""
    ref = lambda c: C.byref(c) if c is not None else None
    kept = C.c_uint64()
    check(lib().pqps_group_head_sort(ctx.h, ref(key_col), int(key_signed), int(descending), ref(group_col), int(group_signed), ids_dev, n,
                                     id_base, limit, int(repeats), out_ids_dev, out_keys_dev, C.byref(kept), stream), "pqps_group_head_sort")
    return int(kept.value)


def count_many_pack(queries, max_queries=COUNT_MANY_MAX):
    """hipCountManyPack: queries = [(Predicate, [column id per slot]), ...], one-pass predicates as compile_plan leaves them.
    -> (batches, places): batches = [(CountMany, [column id per slot of the batch]), ...]; places[i] = (batch, position) of
    query i, (COUNT_CONSTANT, truth value) or (COUNT_ALONE, 0).  Raises ValueError where the packer refuses (reason on
    stderr)."""
    n = len(queries)
    arr = (CountPackQuery * max(1, n))()
    keep = []
    for i, (pred, ids) in enumerate(queries):
        cid = (C.c_int * MAX_COLUMNS)(*([-1] * MAX_COLUMNS))
        for k, c in enumerate(ids):
            cid[k] = c
        keep.append(cid)
        arr[i].pred = C.pointer(pred)
        arr[i].column_ids = C.cast(cid, C.POINTER(C.c_int))
    batches = (CountBatch * max(1, n))()
    places = (CountPlace * max(1, n))()
    nb = C.c_int(0)
    if lib().hipCountManyPack(arr, n, max_queries, batches, C.byref(nb), places) != 0:
        raise ValueError("hipCountManyPack refused (reason on stderr)")
    out = []
    for b in range(nb.value):
        prog = CountMany()
        C.memmove(C.byref(prog), C.byref(batches[b].prog), C.sizeof(CountMany))
        out.append((prog, list(batches[b].column_ids[:prog.n_columns])))
    where = []
    for i in range(n):
        pl = places[i]
        where.append((pl.batch, pl.constant if pl.batch == COUNT_CONSTANT else pl.position if pl.batch >= 0 else 0))
    return out, where


def head_merge(shards, limit):
    """hipHeadMerge: shards = [(bins, words, best_or_None), ...] (sequences in ascending (bin, [best,] word) order); returns
    (bins, words, best_or_None) of the kept entries, or raises ValueError where the C function refuses."""
    keep, arr, total, wide = [], (HeadList * max(1, len(shards)))(), 0, False
    for i, (bins, words, best) in enumerate(shards):
        n = len(bins)
        b, w = (C.c_uint32 * max(1, n))(*bins), (C.c_uint64 * max(1, n))(*words)
        e = (C.c_uint64 * max(1, n))(*best) if best is not None else None
        keep.append((b, w, e))
        arr[i] = HeadList(n, b, w, e)
        total += n
        wide = wide or (best is not None and n > 0)
    ob, ow, oe = (C.c_uint32 * max(1, total))(), (C.c_uint64 * max(1, total))(), (C.c_uint64 * max(1, total))()
    n = lib().hipHeadMerge(arr, len(shards), limit, ob, ow, oe)
    if n < 0:
        raise ValueError("hipHeadMerge refused (reason on stderr)")
    return list(ob[:n]), list(ow[:n]), list(oe[:n]) if wide else None


def filter_digit_hist(ctx, cols, n_cols, n_rows, pred, key_col, key_wide, key_base, key_bits, group_col, bin_base, n_bins, slots,
                      prefix_dev, shift, digit_bits, tables_dev, stream=None):
    """pqps_filter_digit_hist: one fused pass of a radix select; `pred` a Predicate (or its byref), `key_col` / `group_col`
    Columns (group_col None: no GROUP BY), prefix_dev None on the first pass."""
    ref = lambda c: C.byref(c) if c is not None else None
    check(lib().pqps_filter_digit_hist(ctx.h, cols, n_cols, n_rows, C.byref(pred) if isinstance(pred, Predicate) else pred,
                                       ref(key_col), int(key_wide), key_base & 0xFFFFFFFFFFFFFFFF, key_bits, ref(group_col), bin_base,
                                       n_bins, slots, prefix_dev, shift, digit_bits, tables_dev, stream), "pqps_filter_digit_hist")


def digit_hist_list(ctx, key_col, key_wide, key_base, key_bits, group_col, bin_base, n_bins, slots, prefix_dev, shift, digit_bits,
                    n_rows, ids_dev, count_dev, capacity, id_base, tables_dev, stream=None):
    """pqps_digit_hist_list: the same tables over an ID list."""
    ref = lambda c: C.byref(c) if c is not None else None
    check(lib().pqps_digit_hist_list(ctx.h, ref(key_col), int(key_wide), key_base & 0xFFFFFFFFFFFFFFFF, key_bits, ref(group_col),
                                     bin_base, n_bins, slots, prefix_dev, shift, digit_bits, n_rows, ids_dev, count_dev, capacity,
                                     id_base, tables_dev, stream), "pqps_digit_hist_list")


def quantile_rank(n, ppm):
    """hipQuantileRank: the 0-based rank of the fraction `ppm` parts per million among n sorted values."""
    return int(lib().hipQuantileRank(n, ppm))


def quantile_digit_bits(bits_left, key_bits, tables):
    """hipQuantileDigitBits: the width of the next digit of a radix select."""
    return int(lib().hipQuantileDigitBits(bits_left, key_bits, tables))


def quantile_pick(tables, digit_bits, prefixes, entries):
    """hipQuantilePick: tables = the group's counts, slot by slot ([n_slots][2^digit_bits], flat or nested); prefixes = the
    slots' prefixes (None: one slot, prefix 0); entries = [(rank, slot), ...].  Returns (digits, ranks_in, next_prefixes,
    next_slots), or raises ValueError where the C function refuses."""
    flat = [int(x) for row in tables for x in (row if hasattr(row, "__len__") else [row])]
    n_slots, n = (len(prefixes) if prefixes is not None else 1), len(entries)
    t = (C.c_uint64 * max(1, len(flat)))(*flat)
    p = (C.c_uint64 * n_slots)(*prefixes) if prefixes is not None else None
    r, s = (C.c_uint64 * max(1, n))(*[e[0] for e in entries]), (C.c_int * max(1, n))(*[e[1] for e in entries])
    dg, ri, nx, ns = (C.c_uint * max(1, n))(), (C.c_uint64 * max(1, n))(), (C.c_uint64 * max(1, n))(), (C.c_int * max(1, n))()
    n_next = C.c_int()
    if len(flat) != n_slots << digit_bits or lib().hipQuantilePick(t, digit_bits, p, n_slots, r, s, n, dg, ri, nx, ns, C.byref(n_next)) != 0:
        raise ValueError("hipQuantilePick refused (reason on stderr)")
    return list(dg[:n]), list(ri[:n]), list(nx[:n_next.value]), list(ns[:n])


def quantile_ppm(fraction):
    """A fraction as exact parts per million: an int IS ppm (0 .. 1 000 000); a float or Fraction in [0, 1] is
    round(x * 1 000 000) and must lie within 1e-9 of that integer.  ValueError otherwise."""
    if isinstance(fraction, bool):
        raise ValueError(f"fraction {fraction!r}: not a number")
    if hasattr(fraction, "__index__"):                       # int, numpy integers
        ppm = fraction.__index__()
    else:
        scaled = fraction * QUANTILE_PPM
        ppm = round(scaled)
        if not 0 <= fraction <= 1 or abs(scaled - ppm) > 1e-9:
            raise ValueError(f"fraction {fraction!r}: not a whole number of parts per million in [0, 1]")
    if not 0 <= ppm <= QUANTILE_PPM:
        raise ValueError(f"fraction {fraction!r}: outside 0 .. 1 000 000 parts per million")
    return int(ppm)


def first_key_decode(kind, descending, word):
    """hipFirstKeyDecode: None for the empty word, else (key, row); ValueError for a kind without such a word."""
    key, row = C.c_longlong(), C.c_uint()
    rc = lib().hipFirstKeyDecode(kind, int(descending), word, C.byref(key), C.byref(row))
    if rc < 0:
        raise ValueError(f"hipFirstKeyDecode: kind {kind} has no one-word key")
    return (int(key.value), int(row.value)) if rc else None


def remap_codes(ctx, src_dev, src_width, dst_dev, dst_width, n, lut_dev, lut_count, form=None, bad_dev=None, stream=None):
    """pqps_remap_codes: dst[i] = lut[src[i]] for i < n; `form` None = the one pqps_remap_form picks for lut_count."""
    if form is None:
        form = lib().pqps_remap_form(lut_count)
    check(lib().pqps_remap_codes(ctx.h, src_dev, src_width, dst_dev, dst_width, n, lut_dev, lut_count, form, bad_dev, stream),
          "pqps_remap_codes")


def merge_dictionaries(old, new, column="user_name"):
    """hipMergeDictionaries: two ascending lists of bytes -> (merged, lut_old, lut_new, identity); `column` names the field of
    `record` the strings have to fit.  Raises PqpsError when the merge is refused (reason on stderr)."""
    a = (C.c_char_p * max(1, len(old)))(*old)
    b = (C.c_char_p * max(1, len(new)))(*new)
    merged = (C.c_char_p * max(1, len(old) + len(new)))()
    count, identity = C.c_int(), C.c_int()
    lut_old = (C.c_uint32 * max(1, len(old)))()
    lut_new = (C.c_uint32 * max(1, len(new)))()
    if lib().hipMergeDictionaries(a, len(old), b, len(new), COL[column], merged, C.byref(count), lut_old, lut_new, C.byref(identity)) != 0:
        raise PqpsError("hipMergeDictionaries refused the lists (reason on stderr)")
    return list(merged[:count.value]), list(lut_old[:len(old)]), list(lut_new[:len(new)]), bool(identity.value)


def order_keys(keys):
    """A key list -- column names or (column, descending) pairs -- as (hipOrderKey array, count)."""
    pairs = [(k, False) if isinstance(k, (str, bytes)) else (k[0], bool(k[1])) for k in keys]
    arr = (OrderKey * max(1, len(pairs)))()
    for i, (name, desc) in enumerate(pairs):
        arr[i].column = name.encode() if isinstance(name, str) else name
        arr[i].descending = desc
    return arr, len(pairs)


def order_key_plan(keys, dict_counts=None, bounds=None):
    """hipOrderKeyPlan: `keys` as order_keys takes them, dict_counts {column: count}, bounds {column: (lo, hi)} ->
    dict(form, total_bits, fields=[dict(column, kind, descending, base, bits, shift), ...]).  Raises PqpsError when the key
    list is refused (reason on stderr)."""
    pairs = [(k, False) if isinstance(k, (str, bytes)) else (k[0], bool(k[1])) for k in keys]
    names = (C.c_char_p * max(1, len(pairs)))(*[n.encode() if isinstance(n, str) else n for n, _ in pairs])
    desc = (C.c_int * max(1, len(pairs)))(*[int(d) for _, d in pairs])
    counts, lo, hi = (C.c_int * 12)(), (C.c_int * 12)(), (C.c_int * 12)()
    for name, count in (dict_counts or {}).items():
        counts[COL[name]] = count
    for name, (l, h) in (bounds or {}).items():
        lo[COL[name]], hi[COL[name]] = l, h
    plan = OrderKeyPlan()
    if lib().hipOrderKeyPlan(names, desc, len(pairs), counts, lo, hi, C.byref(plan)) != 0:
        raise PqpsError("hipOrderKeyPlan refused the key list (reason on stderr)")
    fields = [dict(column=f.column, kind=f.kind, descending=bool(f.descending), base=f.base, bits=f.bits, shift=f.shift)
              for f in plan.field[:plan.n_fields]]
    return dict(form=plan.form, total_bits=plan.total_bits, fields=fields)


def order_fields(fields):
    """[(Column, base, bits, shift, descending), ...] as a pqps_order_field array."""
    arr = (OrderField * max(1, len(fields)))()
    for i, (col, base, bits, shift, desc) in enumerate(fields):
        arr[i].col, arr[i].base, arr[i].bits, arr[i].shift, arr[i].descending = col, base, bits, shift, int(desc)
    return arr


def filter_topk_multi(ctx, cols, n_cols, n_rows, pred, fields, row_base, k, scratch_dev, scratch_bytes, out_dev, count_dev, stream=None):
    """pqps_filter_topk_multi; `fields` as order_fields takes them.  -> the status (PQPS_OK = 0)."""
    return lib().pqps_filter_topk_multi(ctx.h, cols, n_cols, n_rows, C.byref(pred) if isinstance(pred, Predicate) else pred, order_fields(fields), len(fields), row_base, k,
                                        scratch_dev, scratch_bytes, out_dev, count_dev, stream)


def topk_list_multi(ctx, fields, ids_dev, n, id_base, k, scratch_dev, scratch_bytes, out_dev, stream=None):
    """pqps_topk_list_multi -> the status."""
    return lib().pqps_topk_list_multi(ctx.h, order_fields(fields), len(fields), ids_dev, n, id_base, k, scratch_dev, scratch_bytes,
                                      out_dev, stream)


def sort_list_multi(ctx, fields, ids_dev, n, id_base, out_ids_dev, out_keys_dev=None, stream=None):
    """pqps_sort_list_multi -> the status."""
    return lib().pqps_sort_list_multi(ctx.h, order_fields(fields), len(fields), ids_dev, n, id_base, out_ids_dev, out_keys_dev, stream)


def sort_list_chain(ctx, keys, ids_dev, n, id_base, out_ids_dev, out_keys_dev=None, stream=None):
    """pqps_sort_list_chain; keys: [(Column, key_signed, descending), ...] -> the status."""
    cols = (Column * max(1, len(keys)))()
    for i, (col, _, _) in enumerate(keys):
        cols[i].data, cols[i].width = col.data, col.width
    signed = (C.c_int * max(1, len(keys)))(*[int(sg) for _, sg, _ in keys])
    desc = (C.c_int * max(1, len(keys)))(*[int(d) for _, _, d in keys])
    return lib().pqps_sort_list_chain(ctx.h, cols, signed, desc, len(keys), ids_dev, n, id_base, out_ids_dev, out_keys_dev, stream)


BUCKET_PREFIX, BUCKET_WIDTH = 1, 2                          # HIPBUCKET_* (include/executeEngine-hip.h)


def group_top_order(bins, counts, sums=None, min_images=None, max_images=None, value_kind=-1, by="count", descending=True, limit=10):
    """hipGroupTopOrder: the indices of the listed groups, in order (arrays of u64, any sequence; `by` a TOP_BY name or a
    number).  Raises PqpsError where the function refuses."""
    import numpy as np
    arrays = [None if a is None else np.ascontiguousarray(a, dtype=np.uint64) for a in (bins, counts, sums, min_images, max_images)]
    n = len(arrays[0])
    order = np.zeros(max(n, 1), dtype=np.uint64)
    ptrs = [None if a is None else a.ctypes.data for a in arrays]
    k = lib().hipGroupTopOrder(*ptrs, n, value_kind, TOP_BY.get(by, by), int(bool(descending)), int(limit), order.ctypes.data)
    if k < 0:
        raise PqpsError("hipGroupTopOrder refused (reason on stderr)")
    return [int(i) for i in order[:k]]


def bucket_bounds(column, mode, arg, dictionary=None, lo=0, hi=0):
    """hipBucketBounds: (bounds, keys) of the buckets of `column` -- `dictionary` an ascending list of bytes (BUCKET_PREFIX,
    arg = prefix length) or [lo, hi] the i32 range (BUCKET_WIDTH, arg = width).  bounds: the n + 1 ascending run starts in
    bin space, the last one the domain; keys: the n keys.  Raises PqpsError when it is refused (reason on stderr)."""
    values = list(dictionary) if dictionary is not None else []
    d = (C.c_char_p * max(1, len(values)))(*values)
    bounds, keys, n = C.POINTER(C.c_uint32)(), C.POINTER(C.c_longlong)(), C.c_uint32()
    name = column.encode() if isinstance(column, str) else column
    if lib().hipBucketBounds(name, d if dictionary is not None else None, len(values), lo, hi, mode, arg,
                             C.byref(bounds), C.byref(keys), C.byref(n)) != 0:
        raise PqpsError("hipBucketBounds refused the buckets (reason on stderr)")
    try:
        return list(bounds[:n.value + 1]), list(keys[:n.value])
    finally:
        lib().free(C.cast(bounds, C.c_void_p))
        lib().free(C.cast(keys, C.c_void_p))


# ---- device objects ----------------------------------------------------------------------------
class Context:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        check(lib().pqps_ctx_create(device, C.byref(self.h)), "pqps_ctx_create")

    def info(self):
        name = C.create_string_buffer(64)
        cus, hbm = C.c_int(), C.c_uint64()
        check(lib().pqps_device_info(self.h, name, C.byref(cus), C.byref(hbm)))
        return name.value.decode(), cus.value, hbm.value

    def malloc(self, nbytes):
        p = C.c_void_p()
        check(lib().pqps_malloc(self.h, nbytes, C.byref(p)), "pqps_malloc")
        return p.value

    def free(self, p):
        check(lib().pqps_free(self.h, p))

    def upload(self, dptr, buf, nbytes, stream=None):
        check(lib().pqps_upload(self.h, dptr, buf, nbytes, stream), "pqps_upload")

    def download(self, host, dptr, nbytes, stream=None):
        check(lib().pqps_download(self.h, host, dptr, nbytes, stream), "pqps_download")

    def memset(self, dptr, value, nbytes, stream=None):
        check(lib().pqps_memset(self.h, dptr, value, nbytes, stream))

    def sync(self, stream=None):
        check(lib().pqps_ctx_sync(self.h, stream), "pqps_ctx_sync")

    def pack12(self, codes_dev, n_rows, packed_dev, first_row, padded_rows, stream=None):
        """The 12-bit packed copy (WIDTH_P12) of a u16 device column: rows [first_row rounded down to 8, padded_rows)."""
        check(lib().pqps_pack12(self.h, codes_dev, int(n_rows), packed_dev, int(first_row), int(padded_rows), stream), "pqps_pack12")

    def set_timing(self, on=True):
        check(lib().pqps_ctx_set_timing(self.h, 1 if on else 0))

    def set_option(self, name, value):
        check(lib().pqps_ctx_set_option(self.h, name.encode(), int(value)), "pqps_ctx_set_option")

    def ids_checksum(self, ids_dev, count, stream=None):
        """(sum of ids, sum of ids[i] * (2 i + 1)) mod 2^64 of a device-resident list (pqps_ids_checksum)."""
        out = (C.c_uint64 * 2)()
        check(lib().pqps_ids_checksum(self.h, ids_dev, int(count), out, stream), "pqps_ids_checksum")
        return int(out[0]), int(out[1])

    def kernel_time(self):
        """-> (ms in the scan kernel, ms in the whole query, launches) summed since the last call (an ID query is one launch: both equal)."""
        ev, tot, k = C.c_double(), C.c_double(), C.c_int()
        check(lib().pqps_ctx_kernel_time(self.h, C.byref(ev), C.byref(tot), C.byref(k)))
        return ev.value, tot.value, k.value

    def close(self):
        if self.h:
            lib().pqps_ctx_destroy(self.h)
            self.h = C.c_void_p()


def column_array(pairs):
    """[(device_ptr, width), ...] -> ctypes array of pqps_column."""
    arr = (Column * max(1, len(pairs)))()
    for i, (p, w) in enumerate(pairs):
        arr[i].data, arr[i].width = p, w
    return arr


SYNTH_SHELLS = [b"bash", b"fish", b"sh", b"zsh"]
SYNTH_HOSTS = sorted([b"labpc-01", b"labpc-02", b"labpc-03", b"labpc-04", b"labpc-05", b"labpc-06",
                      b"labpc-07", b"labpc-08", b"labpc-09", b"labpc-10", b"vm-ubuntu-01", b"vm-ubuntu-02",
                      b"cs-lab-01", b"cs-lab-02", b"personal-laptop", b"remote-ssh-01"])
SYNTH_USERS_DICT = [b"student%d" % (1000 + i) for i in range(SYNTH_USERS)]
SYNTH_BASES = sorted(b"cmd%03d" % i for i in range(111))
# the single-valued string columns of the synthetic ENGINE table (initializeEngineSyntheticHIP)
SYNTH_CONSTANTS = {"raw_command": b"cmd", "timestamp": b"2025-01-01T00:00:00.000Z", "working_directory": b"/home/u"}
# (record column, SynthCols field, bytes per row)
SYNTH_LAYOUT = [("command_id", "command_id", 8), ("exit_code", "exit_code", 4), ("user_id", "user_id", 4),
                ("risk_level", "risk_level", 4), ("sudo_used", "sudo_used", 1), ("shell_type", "shell_code", 1),
                ("user_name", "user_code", 2), ("host_name", "host_code", 1), ("base_command", "base_code", 1)]


def synth_schema():
    s = SchemaSpec()
    for name, w in (("command_id", 8), ("exit_code", 4), ("user_id", 4), ("risk_level", 4), ("sudo_used", 1)):
        s.set_numeric(name, w)
    s.set_dict("shell_type", 1, SYNTH_SHELLS)
    s.set_dict("user_name", 2, SYNTH_USERS_DICT)
    s.set_dict("host_name", 1, SYNTH_HOSTS)
    s.set_dict("base_command", 1, SYNTH_BASES)
    return s


def synth_user_tables(seed):
    cdf = (C.c_uint32 * SYNTH_USERS)()
    shell = (C.c_uint8 * SYNTH_USERS)()
    lib().pqps_synth_user_tables(seed, cdf, shell)
    return cdf, shell


class SyntheticTable:
    """Rows [row0, row0+n) of the seeded commands_* table, resident on the device.

    alloc(nbytes) -> device pointer lets the caller own the memory (bench.py passes a
    torch allocator); default is pqps_malloc.  Only `columns` are materialised."""

    def __init__(self, ctx: Context, n_rows, seed=0x5EED, row0=0, columns=None, alloc=None, stream=None):
        self.ctx, self.n, self.seed, self.row0 = ctx, n_rows, seed, row0
        self.schema = synth_schema()
        wanted = set(columns) if columns is not None else {c for c, _, _ in SYNTH_LAYOUT}
        cap = (n_rows + TILE_ROWS - 1) // TILE_ROWS * TILE_ROWS + TILE_ROWS
        self._own = alloc is None
        alloc = alloc or ctx.malloc
        self.ptr, self.width = {}, {}
        sc = SynthCols()
        for name, field, w in SYNTH_LAYOUT:
            if name not in wanted:
                self.schema.schema.col[COL[name]].present = 0
                continue
            p = alloc(cap * w)
            self.ptr[name], self.width[name] = p, w
            setattr(sc, field, p)
        for name in COLUMNS:
            if name not in self.ptr:
                self.schema.schema.col[COL[name]].present = 0
        cdf, shell = synth_user_tables(seed)
        self._cdf_dev, self._shell_dev = ctx.malloc(4 * SYNTH_USERS), ctx.malloc(SYNTH_USERS)
        ctx.upload(self._cdf_dev, cdf, 4 * SYNTH_USERS)
        ctx.upload(self._shell_dev, shell, SYNTH_USERS)
        check(lib().pqps_synth_generate(ctx.h, seed, row0, n_rows, self._cdf_dev, self._shell_dev, C.byref(sc), stream),
              "pqps_synth_generate")
        ctx.sync(stream)

    def bind(self, chain):
        """-> (Predicate, pqps_column array, n_cols, algorithmic bytes per row)."""
        pred, ids = compile_where(self.schema, chain)
        cols = column_array([(self.ptr[COLUMNS[i]], self.width[COLUMNS[i]]) for i in ids])
        return pred, cols, len(ids), sum(self.width[COLUMNS[i]] for i in ids)

    def free(self):
        if self._own:
            for p in self.ptr.values():
                self.ctx.free(p)
        self.ctx.free(self._cdf_dev)
        self.ctx.free(self._shell_dev)
        self.ptr = {}


class ValueSet:
    """A value set of an engine (hipEngineCreateSetHIP): the values of `column` that the rows of an inner WHERE carry,
    optionally filtered by a HAVING, kept on the device.  `item()` is the chain item that tests a column against it."""

    def __init__(self, engine, handle, column):
        self.engine, self._h, self.column = engine, handle, column
        r = handle.contents
        self.id, self.members, self.rows, self.seconds = int(r.id), int(r.members), int(r.rows), float(r.queryTime)

    def item(self, attribute=None, negate=False):
        """(attribute or the set's own column, "IN SET" | "NOT IN SET", str(id))."""
        return (attribute or self.column, "NOT IN SET" if negate else "IN SET", str(self.id))

    def keys(self):
        """hipEngineSetKeysHIP: the members' key texts in key order.  Raises PqpsError for a stale or freed set."""
        if not self._h or not self.engine.e:
            raise PqpsError(f"value set {self.id}: freed")
        res = lib().hipEngineSetKeysHIP(self.engine.e, self._h)
        if not res:
            raise PqpsError(f"value set {self.id}: no keys")
        try:
            r = res.contents
            if not r.success:
                raise PqpsError(f"value set {self.id}: keys refused (reason on stderr)")
            return [r.keyText[g].decode("latin-1") for g in range(r.numKeys)]
        finally:
            lib().freeSetKeysHIP(res)

    def free(self):
        """hipEngineFreeSetHIP; raises PqpsError when refused (the calling thread holds a ticket).  After the engine is
        closed there is nothing left to free."""
        if self._h and lib().hipEngineFreeSetHIP(self.engine.e or None, self._h) != 0:
            raise PqpsError(f"value set {self.id}: free refused (reason on stderr)")
        self._h = None


class HipEngine:
    """initializeEngineHIP / executeQuerySelectHIP / destroyEngineHIP from Python."""

    def __init__(self, csv_path, indexes=()):
        L = lib()
        names = (C.c_char_p * max(1, len(indexes)))(*[a.encode() for a, _ in indexes])
        types = (C.c_int * max(1, len(indexes)))(*[t for _, t in indexes])
        self.e = L.initializeEngineHIP(len(indexes), names, types, str(csv_path).encode(), b"commands")
        self.n = self.e.contents.num_records

    @classmethod
    def _index_args(cls, indexes):
        names = (C.c_char_p * max(1, len(indexes)))(*[a.encode() for a, _ in indexes])
        types = (C.c_int * max(1, len(indexes)))(*[t for _, t in indexes])
        return names, types

    @classmethod
    def synthetic(cls, n_rows, seed=0x5EED, indexes=()):
        """initializeEngineSyntheticHIP: the seeded synthetic table behind the engine API, no host rows."""
        self = cls.__new__(cls)
        names, types = cls._index_args(indexes)
        self.e = lib().initializeEngineSyntheticHIP(n_rows, seed, len(indexes), names, types, b"commands")
        if not self.e:
            raise PqpsError("initializeEngineSyntheticHIP failed")
        self.n = self.e.contents.num_records
        return self

    @classmethod
    def synthetic_rank(cls, rows_total, world, rank, seed=0x5EED):
        """initializeEngineSyntheticRankHIP: this process's rows of a table that `world` processes hold between them
        (not joined yet: join_ranks / join_prepare + join_connect)."""
        self = cls.__new__(cls)
        self.e = lib().initializeEngineSyntheticRankHIP(rows_total, seed, world, rank, b"commands")
        if not self.e:
            raise PqpsError("initializeEngineSyntheticRankHIP failed")
        self.n = self.e.contents.num_records
        return self

    @staticmethod
    def rccl_id(rccl_library):
        ident = C.create_string_buffer(128)
        if lib().hipEngineRcclIdHIP(str(rccl_library).encode(), ident) != 0:
            raise PqpsError("hipEngineRcclIdHIP failed: " + lib().pqps_last_error().decode())
        return ident.raw

    def join_prepare(self, rccl_library):
        if lib().hipEngineJoinPrepareHIP(self.e, str(rccl_library).encode()) != 0:
            raise PqpsError("hipEngineJoinPrepareHIP failed: " + lib().pqps_last_error().decode())

    def join_connect(self, ident):
        if lib().hipEngineJoinConnectHIP(self.e, C.create_string_buffer(ident, 128)) != 0:
            raise PqpsError("hipEngineJoinConnectHIP failed: " + lib().pqps_last_error().decode())

    def join_ranks(self, rccl_library, ident):
        self.join_prepare(rccl_library)
        self.join_connect(ident)

    def leave_ranks(self):
        lib().hipEngineLeaveRanksHIP(self.e)

    def wire_bytes(self, reset=False):
        out = (C.c_ulonglong * 2)()
        lib().hipEngineWireBytesHIP(self.e, out, 1 if reset else 0)
        return int(out[0]), int(out[1])

    def eager_queries(self, reset=False):
        """(SELECTs answered in the sizes all-gather alone, SELECTs finished, IDs a rank's block has room for) of this rank's exchange."""
        out = (C.c_ulonglong * 3)()
        lib().hipEngineEagerQueriesHIP(self.e, out, 1 if reset else 0)
        return int(out[0]), int(out[1]), int(out[2])

    def ticket_checksum(self, ticket):
        """(sum of the row numbers, sum of id[i] * (2 i + 1)) mod 2^64 of the ticket's answer, computed on the device."""
        out = (C.c_ulonglong * 2)()
        if lib().hipQueryChecksumHIP(ticket, out) != 0:
            raise PqpsError("hipQueryChecksumHIP failed")
        return int(out[0]), int(out[1])

    @staticmethod
    def _column_data(columns):
        """{name: numpy array} for numeric columns, {name: (codes array or None, [bytes, ...] dictionary)} for string columns
        -> (ctypes array of the 12 struct hipColumnData, what has to stay alive while it is used)."""
        import numpy as np
        arr = (ColumnData * MAX_COLUMNS)()
        keep = []
        for i, name in enumerate(COLUMNS):
            v = columns[name]
            if COLUMN_KIND[i] == KIND_DICT:
                codes, values = v
                d = (C.c_char_p * max(1, len(values)))(*values)
                keep.append(d)
                arr[i].dictionary, arr[i].dictionary_count = d, len(values)
                if codes is not None:
                    codes = np.ascontiguousarray(codes)
                    keep.append(codes)
                    arr[i].values, arr[i].width = codes.ctypes.data, codes.dtype.itemsize
            else:
                a = np.ascontiguousarray(v)
                keep.append(a)
                arr[i].values, arr[i].width = a.ctypes.data, a.dtype.itemsize
        return arr, keep

    @classmethod
    def from_columns(cls, n_rows, columns, indexes=()):
        """initializeEngineColumnsHIP.  columns: {name: numpy array} for numeric columns,
        {name: (codes array or None, [bytes, ...] dictionary)} for string columns (all 12 of them)."""
        self = cls.__new__(cls)
        arr, keep = cls._column_data(columns)
        names, types = cls._index_args(indexes)
        self.e = lib().initializeEngineColumnsHIP(n_rows, arr, len(indexes), names, types, b"commands")
        if not self.e:
            raise PqpsError("initializeEngineColumnsHIP failed")
        self.n = self.e.contents.num_records
        return self

    def insert_columns(self, n_rows, columns):
        """executeQueryInsertColumnsHIP: appends n_rows rows given as the `columns` dict of from_columns (the batch's own
        dictionaries and codes); -> rows appended.  Raises PqpsError when the batch is refused (nothing changed)."""
        arr, keep = self._column_data(columns)
        k = lib().executeQueryInsertColumnsHIP(self.e, b"commands", n_rows, arr, None)
        self.n = self.e.contents.num_records
        if k < 0:
            raise PqpsError("executeQueryInsertColumnsHIP refused the batch (reason on stderr)")
        return int(k)

    def insert_rows(self, records):
        """executeQueryInsertRowsHIP: appends a list of Record (or a ctypes array of them); -> rows appended.  Raises
        PqpsError when the batch is refused (nothing changed)."""
        rows = records if isinstance(records, C.Array) else (Record * max(1, len(records)))(*records)
        k = lib().executeQueryInsertRowsHIP(self.e, b"commands", rows, len(records), None)
        self.n = self.e.contents.num_records
        if k < 0:
            raise PqpsError("executeQueryInsertRowsHIP refused the batch (reason on stderr)")
        return int(k)

    def select_async(self, chain, count_only=False):
        """-> ticket (opaque).  The WHERE list only has to live until this call returns."""
        wl = WhereList(chain)
        f = lib().executeQueryCountAsyncHIP if count_only else lib().executeQuerySelectAsyncHIP
        return f(self.e, wl.ptr)

    def await_ticket(self, ticket):
        """-> (count, DeviceResult)."""
        res = DeviceResult()
        k = lib().awaitQueryHIP(ticket, C.byref(res))
        return k, res

    def release_ticket(self, ticket):
        lib().releaseQueryHIP(ticket)

    def select_ids(self, chain):
        wl = WhereList(chain)
        ids = C.POINTER(C.c_uint)()
        qt = C.c_double()
        k = lib().executeQuerySelectIdsHIP(self.e, wl.ptr, C.byref(ids), C.byref(qt))
        if k < 0:
            raise PqpsError("executeQuerySelectIdsHIP failed")
        out = list(ids[:k])
        lib().free(ids)
        return out

    def probe_bool_indexes(self, enable=True):
        """Index mode follows QPEOMP / QPEMPI (BOOL indexes probed too, omp:424-459) instead of QPESeq; -> previous setting."""
        return lib().hipEngineProbeBoolIndexes(self.e, 1 if enable else 0)

    def shards(self):
        """Rows held by each device shard (one entry unless PQPS_DEVICES names several devices)."""
        rows = (C.c_ulonglong * 16)()
        k = lib().hipEngineShards(self.e, rows, 16)
        return list(rows[:k])

    def count(self, chain):
        wl = WhereList(chain)
        return lib().executeQueryCountHIP(self.e, wl.ptr)

    def count_many(self, chains):
        """executeQueryCountManyHIP: -> [COUNT(*) of every chain (None: every row)], each what count(chain) gives on the same
        table state; the chains that bind to one scan pass of at most 6 comparisons share their scans, 16 to a launch.
        Raises PqpsError where the engine refuses the call (reason on stderr)."""
        lists = [WhereList(chain) for chain in chains]
        n = len(lists)
        W = C.POINTER(WhereClause)
        ptrs = (W * max(1, n))()
        for i, wl in enumerate(lists):
            if wl.head is not None:
                ptrs[i] = C.pointer(wl.head)
        counts = (C.c_longlong * max(1, n))()
        if lib().executeQueryCountManyHIP(self.e, ptrs, n, counts) != n:
            raise PqpsError("executeQueryCountManyHIP failed")
        return list(counts[:n])

    def value_set(self, column, chain=None, having=None):
        """hipEngineCreateSetHIP: the ValueSet of the values of `column` over the rows for which `chain` is true (None: every
        row; scan semantics, each row once).  having = ("count" | "sum" | "min" | "max", value_column | None, op, constant)
        keeps the values whose aggregate over those rows satisfies `op constant`.  Raises PqpsError when the engine refuses
        (reason on stderr)."""
        wl = WhereList(chain)
        hv = None
        if having is not None:
            agg, vcol, op, const = having
            hv = SetHaving(TOP_BY.get(agg, agg), vcol.encode() if vcol else None, str(op).encode(), str(const).encode())
        res = lib().hipEngineCreateSetHIP(self.e, column.encode(), wl.ptr, C.byref(hv) if hv is not None else None)
        if not res:
            raise PqpsError(f"value_set({column!r}): no result")
        if not res.contents.success:
            lib().hipEngineFreeSetHIP(self.e, res)
            raise PqpsError(f"value_set({column!r}, having={having!r}) refused or failed (reason on stderr)")
        return ValueSet(self, res, column)

    def in_select(self, attribute, column, chain=None, having=None, negate=False):
        """The chain item `attribute [NOT] IN (SELECT column FROM commands WHERE chain [GROUP BY column HAVING having])`: makes
        the value set and keeps it alive with the engine (close() frees it)."""
        vs = self.value_set(column, chain, having)
        if not hasattr(self, "_kept_sets"):
            self._kept_sets = []
        self._kept_sets.append(vs)
        return vs.item(attribute, negate)

    def group_count(self, column, chain=None):
        """executeQueryGroupCountHIP: [(key_text, count), ...] in key order for the rows select_ids(chain) returns,
        grouped by `column`.  Raises PqpsError when the engine refuses (reason on stderr)."""
        wl = WhereList(chain)
        res = lib().executeQueryGroupCountHIP(self.e, column.encode(), wl.ptr)
        if not res:
            raise PqpsError(f"group_count({column!r}): no result")
        try:
            r = res.contents
            if not r.success:
                raise PqpsError(f"group_count({column!r}) refused or failed (reason on stderr)")
            return [(r.keyText[g].decode("latin-1"), int(r.counts[g])) for g in range(r.numGroups)]
        finally:
            lib().freeGroupResultHIP(res)

    def aggregate(self, value_column, group_column=None, chain=None):
        """executeQueryAggregateHIP: [(key_text, count, sum, min, max), ...] of `value_column` over the rows select_ids(chain)
        returns -- in the key order of group_count(group_column, chain), or one entry with key_text None without a group
        column (none when no row matches).  Python ints; command_id's sum (mod 2^64), min and max are unsigned.  Raises
        PqpsError when the engine refuses (reason on stderr)."""
        wl = WhereList(chain)
        res = lib().executeQueryAggregateHIP(self.e, value_column.encode(), group_column.encode() if group_column else None, wl.ptr)
        what = f"aggregate({value_column!r}, {group_column!r})"
        if not res:
            raise PqpsError(f"{what}: no result")
        try:
            r = res.contents
            if not r.success:
                raise PqpsError(f"{what} refused or failed (reason on stderr)")
            fix = (lambda x: x & 0xFFFFFFFFFFFFFFFF) if r.valueKind == HIPKIND_U64 else int
            return [(r.keyText[g].decode("latin-1") if r.groupColumn >= 0 else None, int(r.counts[g]),
                     fix(r.sums[g]), fix(r.mins[g]), fix(r.maxs[g])) for g in range(r.numGroups)]
        finally:
            lib().freeAggregateResultHIP(res)

    def group_top_result(self, column, value_column=None, by="count", descending=True, limit=10, chain=None):
        """executeQueryGroupTopHIP: {"rows": [(key_text, count[, sum, min, max]), ...], "total", "groups_total"} -- the groups
        of `column` (of any size) over the rows select_ids(chain) returns, ordered by `by` ("key", "count", "sum", "min",
        "max"; ties in ascending key order), the first `limit` of them (limit <= 0 or None: all).  Python ints; command_id's
        sum (mod 2^64), min and max are unsigned.  Raises PqpsError when the engine refuses (reason on stderr)."""
        wl = WhereList(chain)
        what = f"group_top({column!r}, {value_column!r}, by={by!r})"
        res = lib().executeQueryGroupTopHIP(self.e, column.encode(), value_column.encode() if value_column else None,
                                            TOP_BY.get(by, by), bool(descending), int(limit or 0), wl.ptr)
        if not res:
            raise PqpsError(f"{what}: no result")
        try:
            r = res.contents
            if not r.success:
                raise PqpsError(f"{what} refused or failed (reason on stderr)")
            n = r.numGroups
            fields = [[t.decode("latin-1") for t in r.keyText[:n]], r.counts[:n]]
            if r.valueColumn >= 0:
                fields += [r.sums[:n], r.mins[:n], r.maxs[:n]]
                if r.valueKind == HIPKIND_U64:
                    fields[2:] = [[x & 0xFFFFFFFFFFFFFFFF for x in f] for f in fields[2:]]
            rows = list(zip(*fields))
            return {"rows": rows, "total": int(r.total), "groups_total": int(r.groupsTotal), "seconds": float(r.queryTime)}
        finally:
            lib().freeGroupTopResultHIP(res)

    def group_top(self, column, value_column=None, by="count", descending=True, limit=10, chain=None):
        """The rows of group_top_result: [(key_text, count[, sum, min, max]), ...]."""
        return self.group_top_result(column, value_column, by, descending, limit, chain)["rows"]

    def group_buckets(self, column, prefix=None, width=None, value_column=None, chain=None):
        """executeQueryGroupBucketsHIP: the rows select_ids(chain) returns, grouped by the first `prefix` bytes of a string
        column or by floor(value / `width`) of an i32 column (exactly one of the two is given) -- [(key_text, count), ...]
        in key order, or [(key_text, count, sum, min, max), ...] with a `value_column` (Python ints; command_id's unsigned).
        key_text is the truncated string, or the range's lower bound.  Raises PqpsError when the engine refuses (reason on
        stderr)."""
        if (prefix is None) == (width is None):
            raise ValueError("group_buckets: exactly one of prefix / width")
        mode, arg = (BUCKET_PREFIX, prefix) if width is None else (BUCKET_WIDTH, width)
        wl = WhereList(chain)
        res = lib().executeQueryGroupBucketsHIP(self.e, column.encode(), mode, arg, value_column.encode() if value_column else None, wl.ptr)
        what = f"group_buckets({column!r}, prefix={prefix!r}, width={width!r}, {value_column!r})"
        if not res:
            raise PqpsError(f"{what}: no result")
        try:
            r = res.contents
            if not r.success:
                raise PqpsError(f"{what} refused or failed (reason on stderr)")
            texts = [r.keyText[g].decode("latin-1") for g in range(r.numGroups)]
            if r.valueColumn < 0:
                return [(texts[g], int(r.counts[g])) for g in range(r.numGroups)]
            fix = (lambda x: x & 0xFFFFFFFFFFFFFFFF) if r.valueKind == HIPKIND_U64 else int
            return [(texts[g], int(r.counts[g]), fix(r.sums[g]), fix(r.mins[g]), fix(r.maxs[g])) for g in range(r.numGroups)]
        finally:
            lib().freeBucketResultHIP(res)

    def group_pair_total(self, group_columns, value_column=None, chain=None):
        """executeQueryGroupPairHIP: (pairs, total, seconds) -- `pairs` as group_pair() returns them, total =
        select_ids(chain)'s length, seconds = the engine's own queryTime."""
        a, b = group_columns
        wl = WhereList(chain)
        res = lib().executeQueryGroupPairHIP(self.e, a.encode(), b.encode(), value_column.encode() if value_column else None, wl.ptr)
        what = f"group_pair(({a!r}, {b!r}), {value_column!r})"
        if not res:
            raise PqpsError(f"{what}: no result")
        try:
            r = res.contents
            if not r.success:
                raise PqpsError(f"{what} refused or failed (reason on stderr)")
            n = r.numGroups
            ta, tb = r.keyText[0][:n], r.keyText[1][:n]
            texts = [(x.decode("latin-1"), y.decode("latin-1")) for x, y in zip(ta, tb)]
            counts = r.counts[:n]
            if r.valueColumn < 0:
                pairs = list(zip(texts, counts))
            else:
                fix = (lambda x: x & 0xFFFFFFFFFFFFFFFF) if r.valueKind == HIPKIND_U64 else int
                pairs = [(t, c, fix(s), fix(lo), fix(hi)) for t, c, s, lo, hi in zip(texts, counts, r.sums[:n], r.mins[:n], r.maxs[:n])]
            return pairs, int(r.total), float(r.queryTime)
        finally:
            lib().freeGroupPairResultHIP(res)

    def group_pair(self, group_columns, value_column=None, chain=None):
        """GROUP BY two columns: over the rows select_ids(chain) returns, per pair of values of `group_columns` (two names)
        that occurs, ((text_a, text_b), count) -- or ((text_a, text_b), count, sum, min, max) of `value_column` -- in
        ascending order of A's key, then B's (each column in group_count's key order).  Python ints; command_id's sum (mod
        2^64), min and max are unsigned, as aggregate() returns them.  Raises PqpsError when the engine refuses (reason on
        stderr)."""
        return self.group_pair_total(group_columns, value_column, chain)[0]

    def average(self, value_column, group_column=None, chain=None):
        """AVG as sum / count of aggregate(): [(key_text, avg), ...] (the device computes no AVG)."""
        return [(k, s / c) for k, c, s, _, _ in self.aggregate(value_column, group_column, chain)]

    def quantiles_result(self, value_column, fractions, group_column=None, chain=None):
        """quantiles plus the raw fields: (groups, dict(total, passes, seconds))."""
        ppm = [quantile_ppm(f) for f in fractions]
        if not 1 <= len(ppm) <= QUANTILE_MAX_FRACTIONS:
            raise ValueError(f"quantiles: {len(ppm)} fractions, not 1 .. {QUANTILE_MAX_FRACTIONS}")
        wl = WhereList(chain)
        res = lib().executeQueryQuantilesHIP(self.e, value_column.encode(), group_column.encode() if group_column else None,
                                             (C.c_uint * len(ppm))(*ppm), len(ppm), wl.ptr)
        what = f"quantiles({value_column!r}, {group_column!r})"
        if not res:
            raise PqpsError(f"{what}: no result")
        try:
            r = res.contents
            if not r.success:
                raise PqpsError(f"{what} refused or failed (reason on stderr)")
            nf = r.numFractions
            if r.valueKind == HIPKIND_DICT:
                value = lambda i: r.valueText[i].decode("latin-1")
            elif r.valueKind == HIPKIND_BOOL:
                value = lambda i: bool(r.values[i])
            elif r.valueKind == HIPKIND_U64:
                value = lambda i: r.values[i] & 0xFFFFFFFFFFFFFFFF
            else:
                value = lambda i: int(r.values[i])
            groups = [(r.keyText[g].decode("latin-1") if r.groupColumn >= 0 else None, int(r.counts[g]),
                       [value(g * nf + f) for f in range(nf)]) for g in range(r.numGroups)]
            return groups, {"total": int(r.total), "passes": int(r.passes), "seconds": float(r.queryTime)}
        finally:
            lib().freeQuantileResultHIP(res)

    def quantiles(self, value_column, fractions, group_column=None, chain=None):
        """executeQueryQuantilesHIP: exact percentiles (SQL's PERCENTILE_DISC) of `value_column` -- any of the 12 columns, in
        order_ids' ascending order -- over the rows select_ids(chain) returns: [(key_text, n, [value, ...]), ...] in the key
        order of group_count(group_column, chain), or one entry with key_text None without a group column (none when no row
        matches).  `fractions`: 1 .. 16 of them, ints as parts per million (0 .. 1 000 000) or floats / Fractions in [0, 1]
        that are whole parts per million (quantile_ppm); for a group of n rows the value for p is the element at 0-based rank
        max(ceil(p n / 10^6) - 1, 0) of its ascending sort.  Values as aggregate and group_first render them: ints, unsigned
        ints for command_id, the text of a string, False / True.  Raises ValueError for the fractions, PqpsError when the
        engine refuses (reason on stderr)."""
        return self.quantiles_result(value_column, fractions, group_column, chain)[0]

    def median(self, value_column, group_column=None, chain=None):
        """The lower median as quantiles([500 000]): [(key_text, n, value), ...]."""
        return [(k, n, v[0]) for k, n, v in self.quantiles(value_column, [500_000], group_column, chain)]

    def order_ids(self, order_column, chain=None, descending=False, limit=None):
        """executeQueryOrderIdsHIP: (ids, matches) -- the row numbers of the first `limit` rows (all with limit None or <= 0)
        of select_ids(chain) ordered by `order_column` (descending with `descending`), ties by ascending row number;
        matches = len(select_ids(chain)).  Raises PqpsError when the engine refuses (reason on stderr)."""
        wl = WhereList(chain)
        ids = C.POINTER(C.c_uint)()
        matches = C.c_longlong()
        qt = C.c_double()
        n = lib().executeQueryOrderIdsHIP(self.e, wl.ptr, order_column.encode(), bool(descending), int(limit or 0), C.byref(ids),
                                          C.byref(matches), C.byref(qt))
        if n < 0:
            raise PqpsError(f"order_ids({order_column!r}) refused or failed (reason on stderr)")
        out = list(ids[:n])
        lib().free(ids)
        return out, int(matches.value)

    def order_ids_by(self, keys, chain=None, limit=None):
        """executeQueryOrderIdsByHIP: (ids, matches) as order_ids, ordered by up to four keys -- column names or (column,
        descending) pairs, the first the most significant; rows equal in all keys come in ascending row number.  Raises
        PqpsError when the engine refuses (reason on stderr)."""
        wl = WhereList(chain)
        arr, n_keys = order_keys(keys)
        ids = C.POINTER(C.c_uint)()
        matches = C.c_longlong()
        qt = C.c_double()
        n = lib().executeQueryOrderIdsByHIP(self.e, wl.ptr, arr, n_keys, int(limit or 0), C.byref(ids), C.byref(matches), C.byref(qt))
        if n < 0:
            raise PqpsError(f"order_ids_by({list(keys)!r}) refused or failed (reason on stderr)")
        out = list(ids[:n])
        lib().free(ids)
        self.last_query_time = qt.value
        return out, int(matches.value)

    def count_distinct_total(self, value_column, group_column=None, chain=None):
        """executeQueryCountDistinctHIP: ([(key_text, distinct), ...], total) -- the number of different values of
        `value_column` over the rows select_ids(chain) returns, in the key order of group_count(group_column, chain), or one
        entry with key_text None without a group column (none when no row matches); total = select_ids(chain)'s length.
        Raises PqpsError when the engine refuses (reason on stderr)."""
        wl = WhereList(chain)
        res = lib().executeQueryCountDistinctHIP(self.e, value_column.encode(), group_column.encode() if group_column else None, wl.ptr)
        what = f"count_distinct({value_column!r}, {group_column!r})"
        if not res:
            raise PqpsError(f"{what}: no result")
        try:
            r = res.contents
            if not r.success:
                raise PqpsError(f"{what} refused or failed (reason on stderr)")
            return ([(r.keyText[g].decode("latin-1") if r.groupColumn >= 0 else None, int(r.distinct[g])) for g in range(r.numGroups)],
                    int(r.total))
        finally:
            lib().freeDistinctResultHIP(res)

    def count_distinct(self, value_column, group_column=None, chain=None):
        """COUNT(DISTINCT value_column) [GROUP BY group_column]: [(key_text, distinct), ...] (count_distinct_total without
        the total)."""
        return self.count_distinct_total(value_column, group_column, chain)[0]

    def update(self, assignments, chain=None):
        """executeQueryUpdateHIP: UPDATE SET column = value, ... WHERE chain (None: every row); `assignments` is
        {column: str | bytes | int | bool}.  -> the number of rows the WHERE selects.  Raises PqpsError when the engine
        refuses (reason on stderr); the table is unchanged then."""
        wl = WhereList(chain)
        names, values, n = assignment_texts(assignments)
        k = lib().executeQueryUpdateHIP(self.e, b"commands", names, values, n, wl.ptr, None)
        if k < 0:
            raise PqpsError(f"update({sorted(assignments)!r}) refused or failed (reason on stderr)")
        return int(k)

    def select(self, columns, chain):
        wl = WhereList(chain)
        items = (C.c_char_p * max(1, len(columns or [])))(*[c.encode() for c in (columns or [])])
        rs = lib().executeQuerySelectHIP(self.e, items if columns else None, len(columns or []), b"commands", wl.ptr)
        r = rs.contents
        names = [r.columnNames[j].decode() for j in range(r.numColumns)]
        rows = [[r.data[i][j].decode("latin-1") for j in range(r.numColumns)] for i in range(r.numRecords)]
        out = dict(numRecords=r.numRecords, numColumns=r.numColumns, columns=names, rows=rows,
                   success=bool(r.success), queryTime=r.queryTime)
        lib().freeResultSet(rs)
        return out

    def select_columnar(self, columns, chain, text=True):
        """executeQuerySelectColumnarHIP: typed per-column arrays gathered on the device; with text=True
        also every cell as the string hipColumnarCellText makes of it."""
        L = lib()
        wl = WhereList(chain)
        items = (C.c_char_p * max(1, len(columns or [])))(*[c.encode() for c in (columns or [])])
        res = L.executeQuerySelectColumnarHIP(self.e, items if columns else None, len(columns or []), wl.ptr)
        return self._columnar_dict(res, text)

    @staticmethod
    def _columnar_dict(res, text):
        """The dict of select_columnar / select_ordered for a hipColumnarResult (which it keeps as "handle")."""
        import numpy as np
        L = lib()
        r = res.contents
        n, m = r.numRecords, r.numColumns
        dtypes = {0: np.uint64, 1: np.int32, 2: np.uint8, 3: np.uint32}
        out = dict(numRecords=n, numColumns=m, columns=[r.columnNames[j].decode() for j in range(m)],
                   kinds=[r.columnKinds[j] for j in range(m)], values=[], success=bool(r.success), handle=res)
        for j in range(m):
            k = r.columnKinds[j]
            if k < 0 or n == 0 or not r.values[j]:
                out["values"].append(None)
            else:
                dt = np.dtype(dtypes[k])
                out["values"].append(np.frombuffer(C.string_at(r.values[j], n * dt.itemsize), dtype=dt).copy())
        if text:
            rows = []
            for i in range(n):
                row = []
                for j in range(m):
                    p = L.hipColumnarCellText(res, i, j)
                    row.append(C.string_at(p).decode("latin-1"))
                    L.free(p)
                rows.append(row)
            out["rows"] = rows
        return out

    def select_ordered(self, columns, chain, order_column, descending=False, limit=None, text=True):
        """executeQuerySelectOrderedHIP: the dict select_columnar returns, its rows those of order_ids(order_column, chain,
        descending, limit) in that order, plus `matches`.  Raises PqpsError when the engine refuses (reason on stderr)."""
        wl = WhereList(chain)
        items = (C.c_char_p * max(1, len(columns or [])))(*[c.encode() for c in (columns or [])])
        matches = C.c_longlong()
        res = lib().executeQuerySelectOrderedHIP(self.e, items if columns else None, len(columns or []), wl.ptr,
                                                 order_column.encode(), bool(descending), int(limit or 0), C.byref(matches))
        if not res or not res.contents.success:
            if res:
                lib().freeColumnarResultHIP(res)
            raise PqpsError(f"select_ordered({order_column!r}) refused or failed (reason on stderr)")
        out = self._columnar_dict(res, text)
        out["matches"] = int(matches.value)
        return out

    def select_ordered_by(self, columns, chain, keys, limit=None, text=True):
        """executeQuerySelectOrderedByHIP: the dict select_columnar returns, its rows those of order_ids_by(keys, chain,
        limit) in that order, plus `matches`.  Raises PqpsError when the engine refuses (reason on stderr)."""
        wl = WhereList(chain)
        items = (C.c_char_p * max(1, len(columns or [])))(*[c.encode() for c in (columns or [])])
        arr, n_keys = order_keys(keys)
        matches = C.c_longlong()
        res = lib().executeQuerySelectOrderedByHIP(self.e, items if columns else None, len(columns or []), wl.ptr, arr, n_keys,
                                                   int(limit or 0), C.byref(matches))
        if not res or not res.contents.success:
            if res:
                lib().freeColumnarResultHIP(res)
            raise PqpsError(f"select_ordered_by({list(keys)!r}) refused or failed (reason on stderr)")
        out = self._columnar_dict(res, text)
        out["matches"] = int(matches.value)
        return out

    def group_first(self, group_column, order_column, chain=None, descending=False):
        """executeQueryGroupFirstHIP: (groups, total) -- per group of `group_column` (None: one group) among the rows
        select_ids(chain) returns, (key_text_or_None, row, order_text) of the row that comes first in order_ids' order of
        `order_column` (ties to the lowest row number in both directions), in group_count's key order; total =
        len(select_ids(chain)).  Raises PqpsError when the engine refuses (reason on stderr)."""
        return self.group_first_result(group_column, order_column, chain, descending)[:2]

    def group_first_result(self, group_column, order_column, chain=None, descending=False):
        """group_first plus the raw fields: (groups, total, dict(keys, order_keys, seconds, ...))."""
        wl = WhereList(chain)
        res = lib().executeQueryGroupFirstHIP(self.e, group_column.encode() if group_column else None, order_column.encode(),
                                              bool(descending), wl.ptr)
        what = f"group_first({group_column!r}, {order_column!r})"
        if not res:
            raise PqpsError(f"{what}: no result")
        try:
            r = res.contents
            if not r.success:
                raise PqpsError(f"{what} refused or failed (reason on stderr)")
            n = r.numGroups
            grouped = r.groupColumn >= 0
            groups = [(r.keyText[g].decode("latin-1") if grouped else None, int(r.rows[g]), r.orderText[g].decode("latin-1"))
                      for g in range(n)]
            fix = (lambda x: x & 0xFFFFFFFFFFFFFFFF) if r.orderKind == HIPKIND_U64 else int
            raw = dict(keys=[int(r.keys[g]) for g in range(n)] if grouped else None, order_keys=[fix(r.orderKeys[g]) for g in range(n)],
                       group_column=r.groupColumn, group_kind=r.groupKind, order_column=r.orderColumn, order_kind=r.orderKind,
                       descending=bool(r.descending), seconds=float(r.queryTime))
            return groups, int(r.total), raw
        finally:
            lib().freeGroupFirstResultHIP(res)

    def select_group_first(self, columns, chain, group_column, order_column, descending=False, text=True):
        """executeQuerySelectGroupFirstHIP: the dict select_columnar returns, its rows those of group_first(group_column,
        order_column, chain, descending) in that order, plus `matches`.  Raises PqpsError when the engine refuses."""
        wl = WhereList(chain)
        items = (C.c_char_p * max(1, len(columns or [])))(*[c.encode() for c in (columns or [])])
        matches = C.c_longlong()
        res = lib().executeQuerySelectGroupFirstHIP(self.e, items if columns else None, len(columns or []), wl.ptr,
                                                    group_column.encode() if group_column else None, order_column.encode(),
                                                    bool(descending), C.byref(matches))
        if not res or not res.contents.success:
            if res:
                lib().freeColumnarResultHIP(res)
            raise PqpsError(f"select_group_first({group_column!r}, {order_column!r}) refused or failed (reason on stderr)")
        out = self._columnar_dict(res, text)
        out["matches"] = int(matches.value)
        return out

    def group_head(self, group_column, order_column, n, chain=None, descending=False):
        """executeQueryGroupHeadHIP: (groups, total) -- per group of `group_column` (None: one group) among the rows
        select_ids(chain) returns, (key_text_or_None, [(row, order_text), ...]) of its first min(n, rows) rows in order_ids'
        order of `order_column` (ties to the lowest row number in both directions), groups in group_count's key order; total =
        len(select_ids(chain)).  Raises PqpsError when the engine refuses (reason on stderr)."""
        return self.group_head_result(group_column, order_column, n, chain, descending)[:2]

    def group_head_result(self, group_column, order_column, n, chain=None, descending=False):
        """group_head plus the raw arrays: (groups, total, dict(keys, offsets, rows, order_keys, seconds, ...))."""
        wl = WhereList(chain)
        res = lib().executeQueryGroupHeadHIP(self.e, group_column.encode() if group_column else None,
                                             order_column.encode() if order_column else None, bool(descending), int(n), wl.ptr)
        what = f"group_head({group_column!r}, {order_column!r}, {n})"
        if not res:
            raise PqpsError(f"{what}: no result")
        try:
            r = res.contents
            if not r.success:
                raise PqpsError(f"{what} refused or failed (reason on stderr)")
            ng = r.numGroups
            grouped = r.groupColumn >= 0
            offsets = [int(r.offsets[g]) for g in range(ng + 1)]
            rows = [int(r.rows[i]) for i in range(offsets[ng])]
            text = [r.orderText[i].decode("latin-1") for i in range(offsets[ng])]
            groups = [(r.keyText[g].decode("latin-1") if grouped else None,
                       list(zip(rows[offsets[g]:offsets[g + 1]], text[offsets[g]:offsets[g + 1]]))) for g in range(ng)]
            fix = (lambda x: x & 0xFFFFFFFFFFFFFFFF) if r.orderKind == HIPKIND_U64 else int
            raw = dict(keys=[int(r.keys[g]) for g in range(ng)] if grouped else None, offsets=offsets, rows=rows,
                       order_keys=[fix(r.orderKeys[i]) for i in range(offsets[ng])], limit=int(r.limit),
                       group_column=r.groupColumn, group_kind=r.groupKind, order_column=r.orderColumn, order_kind=r.orderKind,
                       descending=bool(r.descending), seconds=float(r.queryTime))
            return groups, int(r.total), raw
        finally:
            lib().freeGroupHeadResultHIP(res)

    def select_group_head(self, columns, chain, group_column, order_column, n, descending=False, text=True):
        """executeQuerySelectGroupHeadHIP: the dict select_columnar returns, its rows those of group_head(group_column,
        order_column, n, chain, descending) in answer order, plus `matches` and `offsets` (numGroups + 1 entries).  Raises
        PqpsError when the engine refuses."""
        wl = WhereList(chain)
        items = (C.c_char_p * max(1, len(columns or [])))(*[c.encode() for c in (columns or [])])
        matches = C.c_longlong()
        offsets = C.POINTER(C.c_longlong)()
        res = lib().executeQuerySelectGroupHeadHIP(self.e, items if columns else None, len(columns or []), wl.ptr,
                                                   group_column.encode() if group_column else None,
                                                   order_column.encode() if order_column else None, bool(descending), int(n),
                                                   C.byref(matches), C.byref(offsets))
        if not res or not res.contents.success:
            if res:
                lib().freeColumnarResultHIP(res)
            if offsets:
                lib().free(C.cast(offsets, C.c_void_p))
            raise PqpsError(f"select_group_head({group_column!r}, {order_column!r}, {n}) refused or failed (reason on stderr)")
        rows, off = int(res.contents.numRecords), [0]
        while off[-1] < rows:                                  # every group has a row: the offsets ascend strictly to numRecords
            off.append(int(offsets[len(off)]))
        lib().free(C.cast(offsets, C.c_void_p))
        out = self._columnar_dict(res, text)
        out["matches"] = int(matches.value)
        out["offsets"] = off
        return out

    def free_columnar(self, out):
        lib().freeColumnarResultHIP(out.pop("handle"))

    def record(self, i):
        return self.e.contents.all_records[i].contents

    def close(self):
        if self.e:
            lib().destroyEngineHIP(self.e)                     # frees the value sets that are left, too
            self.e = None
