"""Loader for libqlzx.so (the HIP product library) and its C ABI (include/qlzx.h).

The library is built in-tree by ``gobeansdb_amd.build`` (hipcc, gfx950).  There
is no CPU codec behind this module: if the shared object is missing the
import of any codec entry point raises, and on a host without a GPU the
compute calls fail loudly (``QlzxError``).
"""
from __future__ import annotations

import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("QLZX_LIB", os.path.join(HERE, "libqlzx.so"))
HEADER = os.path.join(ROOT, "include", "qlzx.h")
HTREE_HEADER = os.path.join(ROOT, "include", "qlzx_htree.h")
HTREE_GET_HEADER = os.path.join(ROOT, "include", "qlzx_htree_get.h")

# enum qlzx_status
OK, E_SIZE_COMPRESSED, E_CORRUPT, E_LEVEL, E_DST_CAP, E_CRC, E_HEADER, E_EMPTY, E_TOO_LARGE, E_MAX_DSIZE, E_RUNTIME = range(11)
STATUS_NAMES = ["OK", "E_SIZE_COMPRESSED", "E_CORRUPT", "E_LEVEL", "E_DST_CAP", "E_CRC",
                "E_HEADER", "E_EMPTY", "E_TOO_LARGE", "E_MAX_DSIZE", "E_RUNTIME"]

# enum qlzx_read_status (qlzx_read_plan's verdict per request)
RD_OK, RD_ALIGN, RD_EOF_HEADER, RD_KEY_SIZE, RD_VALUE_SIZE, RD_EOF_BODY, RD_CRC = range(7)
RD_NAMES = ["RD_OK", "RD_ALIGN", "RD_EOF_HEADER", "RD_KEY_SIZE", "RD_VALUE_SIZE", "RD_EOF_BODY", "RD_CRC"]
# enum qlzx_write_status (qlzx_write_plan / qlzx_write_finish's verdict per record)
WR_OK, WR_KEY_SIZE, WR_VALUE_SIZE, WR_NO_SPACE = range(4)
WR_NAMES = ["WR_OK", "WR_KEY_SIZE", "WR_VALUE_SIZE", "WR_NO_SPACE"]
# enum qlzx_gc_status (qlzx_gc_plan / qlzx_gc_rewrite's verdict per record)
GC_WRITTEN, GC_DROPPED, GC_BAD_RECORD, GC_NO_CHUNK, GC_NO_SPACE = range(5)
GC_NAMES = ["GC_WRITTEN", "GC_DROPPED", "GC_BAD_RECORD", "GC_NO_CHUNK", "GC_NO_SPACE"]
# qlzx_hint_plan / qlzx_hint_write: the entries of totals[10], and totals[8]'s QLZX_HINT_NO_SPACE
HINT_CONSUMED, HINT_NUM_KEY, HINT_N_INDEX, HINT_DATASIZE, HINT_INDEX_OFF_LO, HINT_INDEX_OFF_HI, HINT_BYTES_LO, \
    HINT_BYTES_HI, HINT_STATUS, HINT_SKIPPED = range(10)
HINT_NO_SPACE = 1
HINT_SPLIT_CAP = 1 << 20        # store/config_default.go:28 (SplitCapStr "1M")
HINT_INDEX_INTERVAL = 4 << 10   # store/config_default.go:29 (IndexIntervalSizeStr "4K")
# qlzx_hint_merge_plan / qlzx_hint_merge_write: enum qlzx_hm_status (totals[8]) and the entries of
# totals[12]; entries 1..8 sit where qlzx_hint_plan has them
HM_OK, HM_NO_SPACE, HM_BAD_FILE, HM_TOO_MANY, HM_UNSORTED = range(5)
HM_NAMES = ["HM_OK", "HM_NO_SPACE", "HM_BAD_FILE", "HM_TOO_MANY", "HM_UNSORTED"]
HM_ITEMS_READ, HM_NUM_KEY, HM_N_INDEX, HM_DATASIZE, HM_INDEX_OFF_LO, HM_INDEX_OFF_HI, HM_BYTES_LO, HM_BYTES_HI, \
    HM_STATUS, HM_STATUS_SOURCE, HM_N_COLLISION = range(11)
# qlzx_hint_lookup: enum qlzx_hl_status (per request), the entries of totals[4], file_flags and flags
HL_MISS, HL_FOUND, HL_ERR, HL_BAD_FILE = range(4)
HL_NAMES = ["HL_MISS", "HL_FOUND", "HL_ERR", "HL_BAD_FILE"]
HL_N_FOUND, HL_N_MISS, HL_N_ERR, HL_N_BAD_FILE = range(4)
HL_FILE_MERGED = 1
HL_F_BOUNDED, HL_F_LANE, HL_F_WAVE = 1, 2, 4
HL_LANE_FROM = 16384            # QLZX_HL_LANE_FROM: a lane per request from this many on
# qlzx_htree_plan / qlzx_htree_write (include/qlzx_htree.h): enum qlzx_ht_status (totals[8]), the
# entries of totals[10], and what store/config.go:12 and store/htree.go:15-18 fix
HT_OK, HT_NO_SPACE, HT_BAD_FILE, HT_TOO_MANY = range(4)
HT_NAMES = ["HT_OK", "HT_NO_SPACE", "HT_BAD_FILE", "HT_TOO_MANY"]
HT_OPS_READ, HT_N_SET, HT_N_REMOVE, HT_N_SLOTS, HT_N_LEAF, HT_BYTES_LO, HT_BYTES_HI, HT_STATUS_SOURCE, \
    HT_STATUS = range(9)
HT_KHASH_LENS = (8, 8, 7, 7, 6, 6, 5, 5)
HT_MAX_DEPTH, HT_MAX_HEIGHT = 2, 6
HT_LIST_THRESHOLD = 256         # thresholdListKey: a node with fewer items lists them
# include/qlzx_htree_get.h: enum qlzx_htg_status (qlzx_htree_get's verdict per key) and its
# totals[2]; enum qlzx_htg_file and the entries of qlzx_htree_index's totals[4]; the get's flags
HTG_MISS, HTG_FOUND = range(2)
HTG_NAMES = ["HTG_MISS", "HTG_FOUND"]
HTG_N_FOUND, HTG_N_MISS = range(2)
HTG_OK, HTG_BAD_FILE = range(2)
HTG_ITEMS, HTG_N_LEAF, HTG_STATUS, HTG_STATUS_LEAF = range(4)
HTG_F_LANE, HTG_F_WAVE = 1, 2
HTG_LANE_FROM = 4096            # QLZX_HTG_LANE_FROM: a lane per key from this many keys on ...
HTG_LANE_LEAF = 64              # QLZX_HTG_LANE_LEAF: ... where the image holds at most this many items per leaf
HTG_LANE_PER_ITEM = 256         # QLZX_HTG_LANE_PER_ITEM: ... and from this many keys per item of a leaf on
HTG_NO_SLOT = 0xFFFFFFFF
# enum qlzx_gl_verdict (qlzx_gc_liveness's verdict per record), the entries of its totals[8], its flag
GL_BAD, GL_NEWEST, GL_OTHER_POS, GL_NOT_IN_TREE = range(4)
GL_NAMES = ["GL_BAD", "GL_NEWEST", "GL_OTHER_POS", "GL_NOT_IN_TREE"]
GL_N_RECORDS, GL_N_NEWEST, GL_N_OTHER_POS, GL_N_OTHER_POS_DELETED, GL_N_NOT_IN_TREE, GL_N_NOT_IN_TREE_KEPT, \
    GL_N_BAD, GL_N_KEEP = range(8)
GL_F_BEGIN_GT_0 = 1
HTM_MOVED, HTM_SKIPPED = range(2)   # qlzx_htree_move's totals[2]
MAX_NUM_CHUNK = 998  # store/data.go:15: the most destination chunks qlzx_gc_plan takes
# QLZX_NC_*: one bit per audio/video row of http.DetectContentType's table, in record._AV_SIGS
# order, and one for every other answer
NC_AUDIO_BASIC, NC_AUDIO_AIFF, NC_AUDIO_MPEG, NC_APPLICATION_OGG, NC_AUDIO_MIDI, NC_VIDEO_AVI, NC_AUDIO_WAVE, \
    NC_OTHER = (1 << k for k in range(8))
NC_DEFAULT = NC_AUDIO_MPEG | NC_AUDIO_WAVE
# enum qlzx_return
R_OK, R_BAD_ARG, R_WORKSPACE, R_HIP, R_NO_DEVICE = 0, -1, -2, -3, -4

F_GO_COMPAT = 1
F_LEVEL1 = 2
GO_ERROR = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1   # QLZX_GO_ERROR, (size_t)-1


class QlzxError(RuntimeError):
    pass


class Blocks(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("src_off", ctypes.c_void_p),
                ("src_len", ctypes.c_void_p), ("dst", ctypes.c_void_p),
                ("dst_off", ctypes.c_void_p), ("n", ctypes.c_uint32)]


_lib = None


def header_functions(header: str = HEADER) -> list[str]:
    """Every function declared in include/qlzx.h (or in another header of the ABI)."""
    text = open(header).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)   # preprocessor lines (#define X (...))
    return sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)))


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QlzxError(f"{LIB_PATH} is missing: run gobeansdb_amd.build.build() (hipcc, gfx950)")
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, u32, i32, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64
    L.qlz_size_decompressed.argtypes = [vp]
    L.qlz_size_decompressed.restype = sz
    L.qlz_size_compressed.argtypes = [vp]
    L.qlz_size_compressed.restype = sz
    L.qlz_decompress.argtypes = [vp, vp, vp]
    L.qlz_decompress.restype = sz
    L.qlz_compress.argtypes = [vp, vp, sz, vp]
    L.qlz_compress.restype = sz
    L.qlz_get_setting.argtypes = [ctypes.c_int]
    L.qlz_get_setting.restype = ctypes.c_int
    L.crc32_write.argtypes = [u32, vp, ctypes.c_int]
    L.crc32_write.restype = u32
    BP = ctypes.POINTER(Blocks)
    L.qlzx_decompress_workspace_size.argtypes = [u32, u32]
    L.qlzx_decompress_workspace_size.restype = sz
    L.qlzx_decompress_batch.argtypes = [BP, vp, vp, vp, vp, vp, vp, u32, vp, sz, vp]
    L.qlzx_decompress_batch.restype = ctypes.c_int
    L.qlzx_compress_workspace_size.argtypes = [u32, u32]
    L.qlzx_compress_workspace_size.restype = sz
    L.qlzx_compress_batch.argtypes = [BP, vp, vp, vp, vp, u32, u32, vp, sz, vp]
    L.qlzx_compress_batch.restype = ctypes.c_int
    L.qlzx_compress1.argtypes = [vp, vp, sz, u32]
    L.qlzx_compress1.restype = sz
    L.qlzx_go_l1_workspace_size.argtypes = [u32]
    L.qlzx_go_l1_workspace_size.restype = sz
    L.qlzx_go_decompress_workspace_size.argtypes = [u32]
    L.qlzx_go_decompress_workspace_size.restype = sz
    L.qlzx_go_l1_compress_batch.argtypes = [BP, vp, vp, vp, sz, vp]
    L.qlzx_go_l1_compress_batch.restype = ctypes.c_int
    L.qlzx_go_decompress_batch.argtypes = [BP, vp, vp, vp, vp, sz, vp]
    L.qlzx_go_decompress_batch.restype = ctypes.c_int
    L.qlzx_go_decompress1.argtypes = [vp, sz, vp, sz]
    L.qlzx_go_decompress1.restype = sz
    L.qlzx_crc32_batch.argtypes = [vp, vp, vp, u32, vp, u32, vp, vp]
    L.qlzx_crc32_batch.restype = ctypes.c_int
    L.qlzx_synth_batch.argtypes = [ctypes.c_int, u64, u64, vp, vp, vp, u32, vp, vp, vp, u32, vp]
    L.qlzx_synth_batch.restype = ctypes.c_int
    L.qlzx_crc32_combine.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    L.qlzx_crc32_combine.restype = ctypes.c_int
    L.qlzx_copy_batch.argtypes = [vp, vp, vp, vp, vp, u32, vp]
    L.qlzx_copy_batch.restype = ctypes.c_int
    L.qlzx_replay_workspace_size.argtypes = [u64]
    L.qlzx_replay_workspace_size.restype = sz
    L.qlzx_replay_index.argtypes = [vp, u64, u64, u32, u64, vp, vp, vp, vp, sz, vp]
    L.qlzx_replay_index.restype = ctypes.c_int
    L.qlzx_replay_plan_workspace_size.argtypes = [u32]
    L.qlzx_replay_plan_workspace_size.restype = sz
    L.qlzx_replay_plan.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.qlzx_replay_plan.restype = ctypes.c_int
    L.qlzx_replay_finish.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.qlzx_replay_finish.restype = ctypes.c_int
    L.qlzx_read_plan_workspace_size.argtypes = [u32]
    L.qlzx_read_plan_workspace_size.restype = sz
    L.qlzx_read_plan.argtypes = [vp, u64, vp, u32, u32, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.qlzx_read_plan.restype = ctypes.c_int
    L.qlzx_read_finish.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.qlzx_read_finish.restype = ctypes.c_int
    L.qlzx_write_plan_workspace_size.argtypes = [u32]
    L.qlzx_write_plan_workspace_size.restype = sz
    L.qlzx_write_plan.argtypes = [vp] * 6 + [u32, u32, u64, u32] + [vp] * 7 + [sz, vp]
    L.qlzx_write_plan.restype = ctypes.c_int
    L.qlzx_write_decide.argtypes = [vp, vp, u32] + [vp] * 12 + [sz, vp]
    L.qlzx_write_decide.restype = ctypes.c_int
    L.qlzx_write_finish.argtypes = [vp] * 9 + [u32] + [vp] * 16 + [u64] + [vp] * 8 + [sz, vp]
    L.qlzx_write_finish.restype = ctypes.c_int
    L.qlzx_gc_workspace_size.argtypes = [u32, u32]
    L.qlzx_gc_workspace_size.restype = sz
    L.qlzx_gc_plan.argtypes = [vp, u64, vp, vp, u32, vp, u32, u64, u64, vp, u32] + [vp] * 7 + [sz, vp]
    L.qlzx_gc_plan.restype = ctypes.c_int
    L.qlzx_gc_rewrite.argtypes = [vp, u64, vp, vp, u32, vp, u32, vp, vp, vp, vp, u64, vp, vp, vp, vp, sz, vp]
    L.qlzx_gc_rewrite.restype = ctypes.c_int
    L.qlzx_keyhash_batch.argtypes = [vp, vp, vp, u32, vp, vp]
    L.qlzx_keyhash_batch.restype = ctypes.c_int
    L.qlzx_hint_workspace_size.argtypes = [u32]
    L.qlzx_hint_workspace_size.restype = sz
    L.qlzx_hint_plan.argtypes = [vp, u64, vp, vp, u32, vp, vp, u32, u32, ctypes.c_int64, u32] + [vp] * 6 + [sz, vp]
    L.qlzx_hint_plan.restype = ctypes.c_int
    L.qlzx_hint_write.argtypes = [vp, u64, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, u64, vp, vp, sz, vp]
    L.qlzx_hint_write.restype = ctypes.c_int
    L.qlzx_hint_merge_workspace_size.argtypes = [u64, u32, u32]
    L.qlzx_hint_merge_workspace_size.restype = sz
    L.qlzx_hint_merge_plan.argtypes = [vp, u64, vp, vp, vp, u32, u32, ctypes.c_int64] + [vp] * 7 + [sz, vp]
    L.qlzx_hint_merge_plan.restype = ctypes.c_int
    L.qlzx_hint_merge_write.argtypes = [vp, u64, u32, vp, vp, vp, vp, vp, u64, vp, vp, sz, vp]
    L.qlzx_hint_merge_write.restype = ctypes.c_int
    L.qlzx_hint_lookup_workspace_size.argtypes = [u32, u32]
    L.qlzx_hint_lookup_workspace_size.restype = sz
    L.qlzx_hint_lookup.argtypes = [vp, u64, vp, vp, vp, vp, u32, vp, vp, vp, vp, u32, u32] + [vp] * 9 + [sz, vp]
    L.qlzx_hint_lookup.restype = ctypes.c_int
    L.qlzx_htree_workspace_size.argtypes = [u64, u32, u32, u32]
    L.qlzx_htree_workspace_size.restype = sz
    L.qlzx_htree_plan.argtypes = [vp, u64, vp, vp, vp, u32, u32, u32, u32] + [vp] * 7 + [sz, vp]
    L.qlzx_htree_plan.restype = ctypes.c_int
    L.qlzx_htree_write.argtypes = [vp, u64, u32, u32, u32, vp, vp, vp, vp, vp, vp, u64, vp, vp, sz, vp]
    L.qlzx_htree_write.restype = ctypes.c_int
    L.qlzx_htree_index_workspace_size.argtypes = [u32]
    L.qlzx_htree_index_workspace_size.restype = sz
    L.qlzx_htree_index.argtypes = [vp, u64, u32, u32, vp, vp, vp, sz, vp]
    L.qlzx_htree_index.restype = ctypes.c_int
    L.qlzx_htree_get_workspace_size.argtypes = [u32]
    L.qlzx_htree_get_workspace_size.restype = sz
    L.qlzx_htree_get.argtypes = [vp, u64, vp, u32, u32, vp, vp, vp, vp, u32, u32] + [vp] * 8 + [sz, vp]
    L.qlzx_htree_get.restype = ctypes.c_int
    L.qlzx_gc_liveness_workspace_size.argtypes = [u32]
    L.qlzx_gc_liveness_workspace_size.restype = sz
    L.qlzx_gc_liveness.argtypes = [vp, u64, vp, vp, u32, u32, u64, u32, vp, u64, vp, u32, u32, vp, u32] + [vp] * 8 + \
        [sz, vp]
    L.qlzx_gc_liveness.restype = ctypes.c_int
    L.qlzx_htree_move_workspace_size.argtypes = [u32]
    L.qlzx_htree_move_workspace_size.restype = sz
    L.qlzx_htree_move.argtypes = [vp, u64, vp, u32, u32, vp, u32, vp, vp, vp, vp, vp, vp, u32, vp, vp, sz, vp]
    L.qlzx_htree_move.restype = ctypes.c_int
    L.qlzx_vhash_batch.argtypes = [vp, vp, vp, u32, vp, vp]
    L.qlzx_vhash_batch.restype = ctypes.c_int
    L.qlzx_last_status.argtypes = []
    L.qlzx_last_status.restype = ctypes.c_int
    L.qlzx_last_error.argtypes = []
    L.qlzx_last_error.restype = ctypes.c_char_p
    L.qlzx_info.argtypes = [ctypes.c_char_p, sz]
    L.qlzx_info.restype = ctypes.c_int
    L.qlzx_read_record1.argtypes = [vp, sz, u32, u32, ctypes.c_int, vp, sz, ctypes.POINTER(sz),
                                    ctypes.POINTER(ctypes.c_int32)]
    L.qlzx_read_record1.restype = ctypes.c_int
    L.qlzx_service_test_fault.argtypes = [ctypes.c_int]
    L.qlzx_service_test_fault.restype = ctypes.c_int
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().qlzx_last_error().decode(errors="replace")
        raise QlzxError(f"{what} failed ({rc}): {msg}")


def info() -> str:
    buf = ctypes.create_string_buffer(512)
    lib().qlzx_info(buf, 512)
    return buf.value.decode()
