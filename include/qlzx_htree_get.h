/*
 * include/qlzx_htree_get.h -- queries over a bucket's HTree held as its .hash image in device
 * memory: HTree.load's index, a batched HTree.get, GC's liveness verdicts for a replayed chunk and
 * the position update of the records GC moved.  Part of the C ABI of libqlzx.so, beside
 * qlzx_htree.h, whose geometry (depth, height, L, nleaf) and slot rule are used unchanged.
 *
 * The tree is the image plus leaf_first, nothing else:
 *   - image: the `out` of qlzx_htree_write, or a .hash file uploaded once; 16-B aligned.  Its
 *     layout is that of HTree.dump: {count u32, hash u16} per leaf node, then per leaf a u32 byte
 *     length and its items of L + 11 bytes each {the low L bytes of the keyhash, ver i32,
 *     vhash u16, offset >> 8 in 3 bytes, chunk u16}.
 *   - leaf_first: uint32[nleaf + 1], the exclusive scan of the items per leaf: the plan's
 *     leaf_first, or what qlzx_htree_index makes of an image.  Leaf i's items start at image byte
 *     6 nleaf + 4 (i + 1) + (L + 11) leaf_first[i], at any alignment.
 *
 * Conventions as the other qlzx_hint_* / qlzx_htree_* calls: device pointers only, nothing
 * allocates, every launch goes on `stream`, no host synchronisation, one workspace of exactly the
 * matching *_workspace_size bytes with a 16-B aligned base and no state carried between calls.
 * Argument checks answer QLZX_R_BAD_ARG / QLZX_R_WORKSPACE, naming the function in
 * qlzx_last_error(), before any HIP call; depth outside 0..2 or height outside 1..6 is
 * QLZX_R_BAD_ARG, and so is an image of 2^36 bytes or more.  n == 0 or cap == 0 returns QLZX_R_OK
 * and launches nothing.
 * Whatever the image or the arrays hold (leaf_first included), every load stays inside
 * image[0, bytes) and the arrays, every store inside the arrays, and the move's stores inside the
 * image's leaf section.
 */
#ifndef QLZX_HTREE_GET_H
#define QLZX_HTREE_GET_H
#include "qlzx_htree.h"

#ifdef __cplusplus
extern "C" {
#endif

/* qlzx_htree_get's verdict per key; qlzx_htree_index's totals[2] */
enum qlzx_htg_status { QLZX_HTG_MISS = 0, QLZX_HTG_FOUND };
enum qlzx_htg_file { QLZX_HTG_OK = 0, QLZX_HTG_BAD_FILE };
/* qlzx_htree_get's flags: name one kernel shape (tests, sweeps); neither = by n */
enum { QLZX_HTG_F_LANE = 1, QLZX_HTG_F_WAVE = 2 };
/* a lane per key where the image holds at most LANE_LEAF items per leaf on average
 * (leaf = (bytes - 10 nleaf) / (L + 11) / nleaf) and n is at least LANE_FROM and at least
 * LANE_PER_ITEM * leaf; a wave per key otherwise (the crossovers of profiles/r17_htree_get.json) */
#define QLZX_HTG_LANE_FROM 4096u
#define QLZX_HTG_LANE_LEAF 64u
#define QLZX_HTG_LANE_PER_ITEM 256u
/* qlzx_gc_liveness's verdict per record, and its flag: gc.Begin > 0 */
enum qlzx_gl_verdict { QLZX_GL_BAD = 0, QLZX_GL_NEWEST, QLZX_GL_OTHER_POS, QLZX_GL_NOT_IN_TREE };
enum { QLZX_GL_F_BEGIN_GT_0 = 1 };
#define QLZX_HTG_NO_SLOT 0xFFFFFFFFu

/* HTree.load (store/htree.go:107-144) of an image: leaf_first[nleaf + 1] and
 * totals[4] = {items, nleaf, status, the leaf the status names}.
 * QLZX_HTG_BAD_FILE, naming the lowest such leaf: the image ends before the leaf's length word (an
 * image cut inside the node table names leaf 0) or before the leaf's bytes, as io.ReadFull fails
 * there; or the leaf's length is no multiple of L + 11, which the reference does not check and
 * findInBytes would run off.  leaf_first is then all zeros and items is 0.  Bytes behind the last
 * leaf are ignored.  On the `out` of qlzx_htree_write the result is the plan's leaf_first.
 * The leaf nodes' counts give every length word's place at once where no item has ver < 0; they
 * are used only as far as the length words found there prove them (leaf 0's place is known, and a
 * length word equal to count (L + 11) proves the next place); from the first leaf that does not,
 * one lane walks.  The result never depends on the counts. */
size_t qlzx_htree_index_workspace_size(uint32_t height);
int qlzx_htree_index(const uint8_t *image, uint64_t bytes, uint32_t depth, uint32_t height, uint32_t *leaf_first,
                     uint32_t *totals, void *workspace, size_t workspace_bytes, void *stream);

/* HTree.get (store/htree.go:313-330, SliceHeader.Get, findInBytes, store/leaf.go:81-102,155-164)
 * for n keys, passed as to qlzx_hint_lookup: keyhash, or NULL for getKeyHashDefalut of
 * keys[key_off[r] .. + key_len[r]) computed into the workspace; with keyhash the three key arrays
 * may be NULL.  The leaf of a key comes from the slot rule of qlzx_htree.h; the hit is the lowest
 * item of that leaf whose stored low L bytes equal the key's, both taken through that rule.
 * Per key: status (enum qlzx_htg_status), chunk, offset (the three stored bytes << 8), ver (a
 * ver < 0 item is FOUND with that ver), vhash, slot = the item's index among all items of the
 * image; a miss gets zeros and slot = QLZX_HTG_NO_SLOT.  totals[2] = {found, miss}.
 * `offset` widened to 64 bits is qlzx_read_plan's `offsets`, the same keys its `want_key`. */
size_t qlzx_htree_get_workspace_size(uint32_t n);
int qlzx_htree_get(const uint8_t *image, uint64_t bytes, const uint32_t *leaf_first, uint32_t depth, uint32_t height,
                   const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len, const uint64_t *keyhash,
                   uint32_t n, uint32_t flags, int32_t *status, uint32_t *chunk, uint32_t *offset, int32_t *ver,
                   uint16_t *vhash, uint32_t *slot, uint32_t *totals, void *workspace, size_t workspace_bytes,
                   void *stream);

/* The verdicts of GCMgr.gc (store/gc.go:280-312) for the records of source chunk src_chunk:
 * data / size / rec_off / result / cap / max_key / body_max as for qlzx_gc_plan (result[0], the
 * count, stays on the device), keyhash or NULL for getKeyHashDefalut of the key bytes at
 * rec_off[j] + 24.  Per record j < result[0], decided in this order:
 *   QLZX_GL_BAD          the record fails the size checks that make qlzx_gc_plan say BAD_RECORD;
 *                        nothing past the failing check is read.  keep 0.
 *   QLZX_GL_NEWEST       the key is found at (src_chunk, rec_off[j]).  keep 1; vhash[j] is the
 *                        tree's (meta.ValueHash = treeMeta.ValueHash), slot[j] the item.
 *   QLZX_GL_OTHER_POS    the key is found elsewhere.  keep 0, and j is appended to ask_idx
 *                        (ascending): the records for which the reference asks getCollisionGC.
 *                        A binding without a CollisionTable leaves keep as it stands; tree_ver[j]
 *                        is the item's version (isDeleted = tree_ver < 0).
 *   QLZX_GL_NOT_IN_TREE  keep = (flags & QLZX_GL_F_BEGIN_GT_0) && the record's own ver < 0.
 * vhash / tree_ver / slot of a record whose key is not found are 0 / 0 / QLZX_HTG_NO_SLOT.
 * totals[8] = {records, NEWEST, OTHER_POS, OTHER_POS with tree ver < 0, NOT_IN_TREE, of those
 * kept, BAD, keep set}.  Entries j >= result[0] are not written.  keep feeds qlzx_gc_plan. */
size_t qlzx_gc_liveness_workspace_size(uint32_t cap);
int qlzx_gc_liveness(const uint8_t *data, uint64_t size, const uint64_t *rec_off, const uint32_t *result, uint32_t cap,
                     uint32_t max_key, uint64_t body_max, uint32_t src_chunk, const uint8_t *image, uint64_t bytes,
                     const uint32_t *leaf_first, uint32_t depth, uint32_t height, const uint64_t *keyhash,
                     uint32_t flags, uint8_t *keep, int32_t *verdict, uint16_t *vhash, int32_t *tree_ver,
                     uint32_t *slot, uint32_t *ask_idx, uint32_t *totals, void *workspace, size_t workspace_bytes,
                     void *stream);

/* UpdateHtreePos (store/gc.go:85-94) for a whole chunk, after qlzx_gc_rewrite: for every
 * j < result[0] with verdict[j] == QLZX_GL_NEWEST and gc_status[j] == QLZX_GC_WRITTEN, bytes
 * 6..10 behind the stored keyhash of item slot[j] become new_off[j] >> 8 in three bytes and
 * dst_chunk_id[new_chunk[j]] as u16 (dst_chunk_id: max_chunks entries, the real ids of GC's
 * destination chunks).  Set on a present slot rewrites in place and leaves the leaf's count and
 * hash alone, so the image stays the dump of the reference's tree after the same updates.
 * Skipped and counted, not written: new_off >= 2^32, new_off % 256 != 0, new_chunk >= max_chunks,
 * a chunk id >= 65536, slot[j] outside the image's items.  totals[2] = {moved, skipped}.
 * No two NEWEST records of one chunk share a slot (their offsets differ): the stores need no order. */
size_t qlzx_htree_move_workspace_size(uint32_t cap);
int qlzx_htree_move(uint8_t *image, uint64_t bytes, const uint32_t *leaf_first, uint32_t depth, uint32_t height,
                    const uint32_t *result, uint32_t cap, const int32_t *verdict, const int32_t *gc_status,
                    const uint32_t *slot, const uint32_t *new_chunk, const uint64_t *new_off,
                    const uint32_t *dst_chunk_id, uint32_t max_chunks, uint32_t *totals, void *workspace,
                    size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
