/*
 * include/qlzx_htree.h -- the HTree of a bucket and its .hash dump, built from hint files resident
 * in device memory.  Part of the C ABI of libqlzx.so, in a header of its own beside qlzx.h.
 *
 * What bucket open does after the hint split files exist: updateHtreeFromHint over every file
 * (store/bucket.go:119-151, :207-230: HTree.set for ver > 0, HTree.remove with ChunkID = -1
 * otherwise), HTree.Update (updateNodes, store/htree.go:332-359) and HTree.dump (:146-203), over
 * SliceHeader.Set / Remove (store/leaf.go:120-153).
 *
 * Conventions as the other qlzx_hint_* calls: device pointers only (file_off / file_len /
 * file_chunk included, one entry per source), nothing allocates, every launch goes on `stream`, no
 * host synchronisation and no read-back between plan and write, one workspace of
 * qlzx_htree_workspace_size bytes serves both calls (no state is carried in it: the write itself
 * keeps nothing in it).  The sources are described and read exactly as qlzx_hint_merge_plan's
 * (qlzx.h), listed in the order bucket open applies them: chunk ascending, then split ascending.
 *
 *   - depth in {0, 1, 2} (Conf.TreeDepth: 1 / 16 / 256 buckets), height in [1, 6]
 *     (Conf.TreeHeight), p = depth + height - 1, L = KHASH_LENS[p] of {8,8,7,7,6,6,5,5}
 *     (store/config.go:12,82-96).  An item of a leaf is L + 11 bytes, nleaf = 16^(height-1), the
 *     nodes are (16^height - 1) / 15 and stored level-major: level l starts at (16^l - 1) / 15.
 *     Any other depth or height is QLZX_R_BAD_ARG.
 *   - a source without any item is valid (the reader's loop just ends).  QLZX_HT_BAD_FILE
 *     (totals[7] = the lowest such source): file_len < 16, the source runs past `bytes`,
 *     indexOffset negative or > file_len, or an item that starts below indexOffset ends past the
 *     file.  The reference fails bucket open there.
 *   - ops: the items of all sources, in source order and then file order.  ver > 0 sets the slot
 *     to (file_chunk[source], offset, ver, vhash); ver <= 0 removes it (an absent slot stays
 *     absent).  The key bytes are never read: the keyhash is the stored one.
 *   - the slot of a keyhash is keyhash & (~0 >> 4 depth): the bucket nibbles are ignored, and since
 *     8 L + 4 p >= 64 the rest is exactly (leaf, the low L bytes findInBytes compares).  The leaf is
 *     the slot's top 4 (height - 1) bits below the dropped nibbles.
 *   - a slot is present iff its last op is a set, with that op's data.  Its place in the leaf goes
 *     by its incarnation start: the first set after its last remove (Set on an existing slot
 *     rewrites in place, Remove shifts the tail down, a later Set appends).  A leaf's bytes are its
 *     present slots ascending by incarnation start, each {the low L bytes of the keyhash, ver i32,
 *     vhash u16, offset >> 8 in 3 bytes, chunk u16} (khashToBytes, itemToBytes).
 *   - leaf node: count = its present slots, hash = the sum of vhash * uint16(keyhash >> 32) over
 *     them mod 2^16.  Upper node: count = the sum of its 16 children, hash = the fold over them of
 *     { if count > 256: hash *= 97; hash += child.hash } in uint16, count being the node's own.
 *   - file: {count u32, hash u16} per leaf node, then per leaf a u32 byte length and its bytes:
 *     10 nleaf + (L + 11) slots bytes.
 *   - QLZX_HT_TOO_MANY: the sources hold more than cap items.  Precedence: BAD_FILE, TOO_MANY; with
 *     either every count, node, leaf_first entry and the file bytes are 0 and qlzx_htree_write
 *     writes nothing and keeps the status.
 * The sources' own index sections only cut the (serial) walk over a source into stretches, and only
 * once proven, as for qlzx_hint_merge_plan; the result never depends on an index section.
 * Whatever the bytes or the plan arrays hold, every load stays inside hints[0, bytes) and the
 * arrays, every store inside the arrays and out_cap, and every walk advances 23 bytes or more per
 * step.
 */
#ifndef QLZX_HTREE_H
#define QLZX_HTREE_H
#include "qlzx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum qlzx_ht_status { QLZX_HT_OK = 0, QLZX_HT_NO_SPACE, QLZX_HT_BAD_FILE, QLZX_HT_TOO_MANY };
/* Workspace of the two qlzx_htree_* calls (`bytes` and `height` do not enter it today). */
size_t qlzx_htree_workspace_size(uint64_t bytes, uint32_t n_files, uint32_t cap, uint32_t height);
/* The plan: the tree's nodes and the order of the dump.  cap = the capacity of slot_src /
 * slot_chunk and the most ops the sources may hold.
 *   node_count / node_hash: (16^height - 1) / 15 entries, every level, level-major;
 *   leaf_first: nleaf + 1 entries, the exclusive scan of the present slots per leaf;
 *   slot_src[k]: the byte offset in `hints` of the source item that supplies the data of slot k,
 *   slot_chunk[k]: its chunk, the slots in file order (leaf, then incarnation start);
 *   totals[10] = {ops read, sets, removes, present slots, nleaf, file bytes (lo, hi), the source
 *   the status names, status, 0}.
 * n_files == 0 is a valid empty tree: every node is zero and the file is 10 nleaf bytes.
 * cap == 0 returns QLZX_R_OK; nothing is launched or written. */
int qlzx_htree_plan(const uint8_t *hints, uint64_t bytes, const uint64_t *file_off, const uint64_t *file_len,
                    const uint32_t *file_chunk, uint32_t n_files, uint32_t cap, uint32_t depth, uint32_t height,
                    uint32_t *node_count, uint16_t *node_hash, uint32_t *leaf_first, uint64_t *slot_src,
                    uint32_t *slot_chunk, uint32_t *totals, void *workspace, size_t workspace_bytes, void *stream);
/* The file, after qlzx_htree_plan: 10 nleaf + (L + 11) totals[3] bytes from `out` on.  `out` is
 * 16-B aligned and need not be zeroed; no byte past the file's is written.  If the file exceeds
 * out_cap nothing is written and totals[8] = QLZX_HT_NO_SPACE; a status of the plan stays.
 * 10 nleaf + 19 cap bytes always suffice.  cap == 0 returns QLZX_R_OK. */
int qlzx_htree_write(const uint8_t *hints, uint64_t bytes, uint32_t cap, uint32_t depth, uint32_t height,
                     const uint32_t *node_count, const uint16_t *node_hash, const uint32_t *leaf_first,
                     const uint64_t *slot_src, const uint32_t *slot_chunk, uint8_t *out, uint64_t out_cap,
                     uint32_t *totals /* in/out */, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
