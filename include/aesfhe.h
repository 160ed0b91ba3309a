/*
 * aesfhe.h -- C ABI of the MI355X-native CKKS engine (libaesfhe.so).
 *
 * This is the drop-in boundary for the reference's hot path: every CKKS primitive the
 * reference reaches through EngineContext (REF/engine_context.py:56-204), i.e. through
 * the closed-source `desilofhe.Engine` (REF/engine_context.py:1,17-50), is one entry
 * point here.  Signatures use plain pointers, sizes and opaque 64-bit handles; the
 * Python shim (aes-implementation-fhe_amd/mi355x_ckks.py) binds them with ctypes.
 *
 * Conventions
 *   - Every function returns 0 on success or a negative status; the message is then
 *     available from aesfhe_last_error(ctx).  Level exhaustion messages contain the
 *     word "level" and relinearising a 2-polynomial ciphertext reports
 *     "should have 3 polynomials" (the strings REF/engine_context.py:139-145,186-195
 *     and REF/xor4_lut.py:33-51 branch on).
 *   - Results are always new handles; inputs are never modified.  Free every handle
 *     with aesfhe_free.
 *   - Slots are passed as separate real/imaginary double arrays of slot_count entries.
 *   - rotate(ct, steps) == np.roll(slots, steps)  (SURVEY.md quirk 4e).
 *   - A context is bound to one HIP device and one stream; it is not thread safe, but
 *     independent contexts (one per GPU) are.
 */
#ifndef AESFHE_H
#define AESFHE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aesfhe_ctx aesfhe_ctx;
typedef uint64_t aesfhe_handle;

/* --- context / keys -------------------------------------------------------------- */
/* replaces desilofhe.Engine(...) construction, REF/engine_context.py:17-39 */
int aesfhe_create(aesfhe_ctx** out, int log_n, int max_level, int dnum, int device_id, uint64_t seed);
/* bootstrappable parameter set: fresh ciphertexts at fresh_level, the chain extended by
 * aesfhe_bootstrap_depth() levels (CoeffToSlot/EvalMod on double-prime levels) */
int aesfhe_create_boot(aesfhe_ctx** out, int log_n, int fresh_level, int dnum, int device_id, uint64_t seed);
/* Randomness: every key and encryption sample is a ChaCha20 block under a 256-bit context key
 * (DESIGN.md §3.4).  aesfhe_create / aesfhe_create_boot take a 64-bit seed as key words 0-1
 * (reproducible test and parity contexts); aesfhe_create_keyed takes the full 32-byte key
 * (little-endian words; the Python Engine draws it from os.urandom unless a seed is given).
 * bootstrappable != 0: max_level is the fresh level of a bootstrappable set (aesfhe_create_boot). */
int aesfhe_create_keyed(aesfhe_ctx** out, int log_n, int max_level, int dnum, int device_id, const uint8_t* key,
                        int bootstrappable);
/* Evaluation-only context: the server side of the client/server protocol.  It never holds the
 * secret: the public key and the switching keys come in through aesfhe_import_pk / aesfhe_import_ksk, and prng_key
 * (32 bytes of the caller's OWN randomness, never the client's key) seeds only its encryption samples.  Every call
 * that needs the secret -- aesfhe_keygen, aesfhe_decrypt, every aesfhe_renorm_* entry, aesfhe_export_secret,
 * aesfhe_export_sparse -- fails with "no secret key" in aesfhe_last_error; a key switch whose key was not imported
 * fails with "evaluation key missing: galois <tag>, level <l>" (level -1: the full key) instead of generating it.
 * The context stays usable after either error.  Every other call behaves as on a keyed context. */
int aesfhe_create_eval(aesfhe_ctx** out, int log_n, int max_level, int dnum, int device_id, int bootstrappable,
                       const uint8_t* prng_key);
/* 1: a keyed context, 0: an evaluation-only one (negative: no context) */
int aesfhe_has_secret(aesfhe_ctx* ctx);
/* The switching keys present, generated or imported, as (galois tag, level) pairs; level -1: a full key
 * [dnum][2][n_ks + n_p][N] (the dense -> sparse key of the bootstrap: [2][2 + np'][N]), level >= 0: that reduced
 * level's own key (aesfhe_export_ksk_at).  Writes the first `cap` pairs and returns the count of all (negative on
 * error): call with cap 0 for the count.  A client exports exactly these after a warm-up run of its workload. */
int aesfhe_eval_keys(aesfhe_ctx* ctx, uint64_t* galois, int32_t* level, int cap);
/* uint32 words of the key (galois, level), level -1: the full key; a level >= 0 must be a reduced one */
int aesfhe_ksk_words(aesfhe_ctx* ctx, uint64_t galois, int level, uint64_t* words);
/* Imports into an evaluation-only context: the public key [2][n_q][N] and the key (galois, level) in the layout
 * aesfhe_export_pk / aesfhe_export_ksk / aesfhe_export_ksk_at wrote.  Refused with a message: a wrong word count, a
 * level >= 0 that is not a reduced level under the current aesfhe_set_low_p setting, a key already present, a
 * keyed context, and any residue not below its row's modulus (the device checks every word once; the message
 * names the first such row and nothing is stored). */
int aesfhe_import_pk(aesfhe_ctx* ctx, const uint32_t* data, uint64_t words);
int aesfhe_import_ksk(aesfhe_ctx* ctx, uint64_t galois, int level, const uint32_t* data, uint64_t words);
/* the key (galois, level) made resident without running an operation: generated on a keyed context if absent;
 * on an evaluation-only context a lookup ("evaluation key missing" if absent) */
int aesfhe_ensure_key(aesfhe_ctx* ctx, uint64_t galois, int level);
/* The import check for a ciphertext handle (aesfhe_import itself checks nothing): *bad_row = the first row
 * ([npoly][limbs] order) holding a residue not below its modulus, or -1 when every residue is reduced. */
int aesfhe_check(aesfhe_ctx* ctx, aesfhe_handle handle, int32_t* bad_row);
/* Seed-compressed keys.  The MASK KEY is a second, PUBLIC 256-bit key: once set, the uniform `a`
 * half of the public key and of every switching key is drawn under it (the secret, every error polynomial and the
 * encryption samples stay under the context key), so a key travels as its `b` half and the receiver regenerates `a`
 * on the device.  Without a mask key nothing changes.  aesfhe_set_mask_key is refused with a message: on a keyed
 * context once any key exists (set it before aesfhe_keygen), when it equals the context's own key (publishing that
 * key would publish the secret), and when a mask key is already set.  On an evaluation-only context it is set
 * before the first half import.  aesfhe_has_mask_key: 1 / 0 (negative: no context); aesfhe_mask_key writes its 32
 * bytes. */
int aesfhe_set_mask_key(aesfhe_ctx* ctx, const uint8_t* key);
int aesfhe_has_mask_key(aesfhe_ctx* ctx);
int aesfhe_mask_key(aesfhe_ctx* ctx, uint8_t* out);
/* The `b` halves of a keyed context's keys: [n_q][N] for the public key, [dnum][n_ks + n_p][N] for a full switching
 * key (level -1), [nkey][N] for the dense -> sparse key and for a reduced level's key (level >= 0); `words` is the
 * size of `out` and must be half of aesfhe_ksk_words (of 2 n_q N for the public key).  A switching key that is
 * absent is generated, as by aesfhe_export_ksk.  Refused on a context without a mask key: keys made under the
 * context key cannot be compressed, their `a` halves are not public. */
int aesfhe_export_pk_half(aesfhe_ctx* ctx, uint32_t* out, uint64_t words);
int aesfhe_export_ksk_half(aesfhe_ctx* ctx, uint64_t galois, int level, uint32_t* out, uint64_t words);
/* The same halves into an evaluation-only context that holds the exporter's mask key: the whole key is allocated,
 * the `b` rows are copied into place and one kernel launch checks them and writes every `a` row; the key is then
 * word for word the exporter's (aesfhe_export_ksk on both sides agrees).  Refused as aesfhe_import_pk /
 * aesfhe_import_ksk refuse, and without a mask key; a residue not below its modulus names its row in the half
 * (digit * nkey + row) and stores nothing. */
int aesfhe_import_pk_half(aesfhe_ctx* ctx, const uint32_t* data, uint64_t words);
int aesfhe_import_ksk_half(aesfhe_ctx* ctx, uint64_t galois, int level, const uint32_t* data, uint64_t words);
/* Seeded symmetric encryption, the upload path of the same protocol: c = (e + m - a s, a) at `level`
 * (-1: the fresh level; 0..fresh otherwise) and that level's scale, on exactly its limbs, with no rescale: an ordinary
 * two-polynomial ciphertext, fresher than aesfhe_encrypt's.  `a` is the PRF under the mask key at a 56-bit id
 * (counter << 16) | (encryption nonce & 0xffff), so the ciphertext travels as its `b` rows plus the id.  The counter is
 * the context's own: it starts at 0, advances by `count` per call and is never shared with aesfhe_encrypt's.
 * re, im: `count` messages of slot_count doubles each (im null: real); out: `count` handles, member j's id is the first
 * one's + (j << 16); *id0 (nullable): the first one's.  Refused with a message: without a mask key (an `a` drawn under the context key cannot be
 * published), on an evaluation-only context (no secret key), for a level out of range, for count outside 1..16384 and
 * when the counter would reach 2^40. */
int aesfhe_encrypt_sym(aesfhe_ctx* ctx, const double* re, const double* im, int count, int level, aesfhe_handle* out, uint64_t* id0);
/* The `b` rows [limbs][N] of a handle aesfhe_encrypt_sym returned, and its id; `words` is the size of `out`, half the
 * ciphertext's.  Any other handle is refused ("not a seeded ciphertext"): handles are values, so the result of an
 * operation on a seeded ciphertext, an import and a public-key encryption carry no id. */
int aesfhe_export_half(aesfhe_ctx* ctx, aesfhe_handle handle, uint32_t* out, uint64_t words, uint64_t* id);
/* `count` ciphertexts at `level` from their `b` rows (rows[j]: [limbs][N], `words` words each, wherever each arrived: no
 * gathering copy) and the consecutive ids id0 + (j << 16),
 * on any context that holds the exporter's mask key, an evaluation-only one included: each ciphertext is allocated, its
 * `b` rows are copied into place and one kernel launch (per 32 members) checks them and writes every `a` row; an
 * aesfhe_export of the handle then equals the exporter's word for word.  Refused without a mask key, for a wrong word
 * count, a level out of range, count outside 1..16384 and an id whose counter part would reach 2^40; a residue not
 * below its modulus names member and row and stores nothing. */
int aesfhe_import_half(aesfhe_ctx* ctx, const uint32_t* const* rows, uint64_t words, int level, uint64_t id0, int count, aesfhe_handle* out);
/* Encryption randomness (v, e0, e1 of every encryption, the renorms' re-encryptions included)
 * is drawn under the context key with `nonce` folded into key words 6-7; key material is not
 * affected.  Processes sharing one context key (the ranks of a multi-GPU job) must
 * set different nonces, otherwise their i-th encryptions reuse (v, e) and the difference of two
 * ranks' ciphertexts is a noiseless encoding of the plaintext difference.  Default 0; the Python
 * Engine draws a random one per process (os.urandom) unless pinned.  No reference counterpart:
 * desilofhe.Engine.encrypt (REF/engine_context.py:56-57) samples internally. */
int aesfhe_set_enc_nonce(aesfhe_ctx* ctx, uint64_t nonce);
/* Per-level special basis.  on != 0: a key switch at a level of nl < alpha limbs
 * (one digit) runs over the first nl + 1 special primes only, with that level's own switching keys
 * (generated on first use from the context key, kept resident); levels of nl >= alpha limbs and the
 * bootstrap's linear transforms keep all n_p special primes.  Decoded results are unchanged,
 * ciphertext residues are not (different keys).  Default off (or the environment's AESFHE_LOW_P):
 * every residue is then the full-basis engine's.  Set it before the first key switch it should
 * cover; it may be changed between operations. */
int aesfhe_set_low_p(aesfhe_ctx* ctx, int on);
/* special primes a key switch at `level` runs over under the current setting */
int aesfhe_ks_special_primes(aesfhe_ctx* ctx, int level, int32_t* out);
/* limbs per level 0..max_level (a ciphertext at level l has npoly x limbs[l] x N words) */
int aesfhe_level_limbs(aesfhe_ctx* ctx, int32_t* out);
int aesfhe_destroy(aesfhe_ctx* ctx);
const char* aesfhe_last_error(aesfhe_ctx* ctx);

/* Concurrency (MI355X-side; the reference engine is single-stream).  A context owns
 * aesfhe_streams() HIP streams.  Stream 0 serves every host thread by default; a host
 * thread that calls aesfhe_bind_stream(ctx, k) queues its work on stream k.
 * aesfhe_fork() makes streams 1.. start after all work queued so far on stream 0;
 * aesfhe_join() makes stream 0 continue only after them.  Between fork and join the
 * branches must be independent (they may read handles created before the fork); handles
 * freed by branch threads are recycled at the join.  Calls are serialised by a context
 * mutex and errors are per thread. */
int aesfhe_streams(aesfhe_ctx* ctx);
int aesfhe_bind_stream(aesfhe_ctx* ctx, int index);
int aesfhe_fork(aesfhe_ctx* ctx);
/* applies a handle's deferred work now, so branches that share it read one
 * canonical copy instead of each normalising its own */
int aesfhe_settle(aesfhe_ctx* ctx, aesfhe_handle c);
int aesfhe_join(aesfhe_ctx* ctx);
/* replaces create_secret_key / create_public_key / create_relinearization_key /
 * create_conjugation_key, REF/engine_context.py:44-48 (rotation keys are made on first use) */
int aesfhe_keygen(aesfhe_ctx* ctx);
/* engine.slot_count, read by every module (e.g. REF/state_encoder.py:14) */
int aesfhe_slot_count(aesfhe_ctx* ctx);
int aesfhe_max_level(aesfhe_ctx* ctx);
/* level of fresh encryptions (default max_level; lower when the chain is extended for bootstrapping) */
int aesfhe_set_fresh_level(aesfhe_ctx* ctx, int level);
/* info: [n, L, n_q, n_ks, n_p, alpha, dnum, log_n] */
int aesfhe_info(aesfhe_ctx* ctx, int32_t* info8);
int aesfhe_moduli(aesfhe_ctx* ctx, uint32_t* out);   /* n_q + n_p primes */
int aesfhe_scales(aesfhe_ctx* ctx, double* out);     /* delta_0 .. delta_L */
int aesfhe_sync(aesfhe_ctx* ctx);
int aesfhe_free(aesfhe_ctx* ctx, aesfhe_handle h);
int aesfhe_level(aesfhe_ctx* ctx, aesfhe_handle ct, int32_t* level, int32_t* npoly);

/* --- plaintexts / codec ------------------------------------------------------------ */
/* engine.encode(vec), REF/engine_context.py:62-63 (level-agnostic; encoded on use) */
int aesfhe_plaintext(aesfhe_ctx* ctx, const double* re, const double* im, int n, aesfhe_handle* out);
/* engine.encrypt(data, public_key), REF/engine_context.py:56-57 */
int aesfhe_encrypt(aesfhe_ctx* ctx, const double* re, const double* im, int n, aesfhe_handle* out);
/* engine.decrypt(ct, secret_key), REF/engine_context.py:59-60 */
int aesfhe_decrypt(aesfhe_ctx* ctx, aesfhe_handle ct, double* re, double* im, int n);

/* --- arithmetic ---------------------------------------------------------------------- */
/* engine.add / engine.subtract, REF/engine_context.py:70-74 (levels auto-aligned) */
int aesfhe_add(aesfhe_ctx* ctx, aesfhe_handle a, aesfhe_handle b, aesfhe_handle* out);
int aesfhe_sub(aesfhe_ctx* ctx, aesfhe_handle a, aesfhe_handle b, aesfhe_handle* out);
/* engine.add(ct, pt) / engine.add_plain(ct, scalar), REF/engine_context.py:76-98 */
int aesfhe_add_pt(aesfhe_ctx* ctx, aesfhe_handle ct, aesfhe_handle pt, aesfhe_handle* out);
int aesfhe_add_scalar(aesfhe_ctx* ctx, aesfhe_handle ct, double re, double im, aesfhe_handle* out);
/* engine.multiply(ct, scalar|pt), REF/engine_context.py:65-68,106-125 */
int aesfhe_mul_scalar(aesfhe_ctx* ctx, aesfhe_handle ct, double re, double im, aesfhe_handle* out);
int aesfhe_mul_pt(aesfhe_ctx* ctx, aesfhe_handle ct, aesfhe_handle pt, aesfhe_handle* out);
/* engine.multiply(a, b, relinearization_key), REF/engine_context.py:65-67:
 * tensor + relinearise + rescale; relin = 0 returns the 3-polynomial tensor (rescaled) */
int aesfhe_mul(aesfhe_ctx* ctx, aesfhe_handle a, aesfhe_handle b, int relin, aesfhe_handle* out);
/* Fused LUT evaluation.  One kernel replaces the per-term product loops of
 *   REF/xor4_lut.py:63-74           XOR4LUT.apply:        sum_{p,q} C[p,q] A^p B^q
 *   REF/mixcol_final.py:80-91       _gf_poly_eval_2var    (same form, GF LUT coefficients)
 *   REF/invmixcolumns_fhe.py:76-87  _poly2_eval           (same form)
 *   REF/sub_bytes_lut.py:46-74      lift / hi / lo sums:  c0 + sum_k C[k] X^k
 *   REF/lut.py:71-94                LUTEvaluator.apply    (same univariate form)
 * lut_create stores the n_a x n_b coefficient matrix (row-major re / im; n_b = 1 makes a
 * univariate LUT with constant term c0; bivariate LUTs are at most 16 x 16).  lut_eval takes
 * the element handles a[0..n_a) (and b[0..n_b) for bivariate LUTs; entries whose coefficients
 * are all zero may be 0) and returns the sum at the logical level of the per-term products
 * (lowest element level - 2, resp. - 1); it fails with a message containing "level" when the
 * elements are too low for the fused form, and the caller falls back to the product loop. */
int aesfhe_lut_create(aesfhe_ctx* ctx, int n_a, int n_b, const double* re, const double* im, double c0_re, double c0_im,
                      aesfhe_handle* out);
int aesfhe_lut_eval(aesfhe_ctx* ctx, aesfhe_handle lut, const aesfhe_handle* a, const aesfhe_handle* b, aesfhe_handle* out);
/* Bivariate LUT(s) with a PUBLIC second operand: out_k = sum_p (sum_q C_k[p,q] zeta16^(q * nib[j])) a[p]
 * at slot j: aesfhe_lut_eval with b an exact Zeta16 codeword known in clear (zeta16 = e^(-2 pi i / 16), the
 * clear value of basis element q at nibble v being zeta16^(q v) for every q, mirrors included).  The XORs of
 * a counter mode -- public counter block with the encrypted round key, encrypted keystream with the public
 * AES ciphertext -- where REF/xor4_lut.py:63-74 would first encrypt the public bytes and form a second
 * power basis; no reference counterpart.  lut1 / lut2 (0 = none): bivariate LUT handles with n_b = 16 and
 * the same n_a, evaluated together (a conjugate-split LUT's S1 and S2): every a[p] is read once for both.
 * a[0..n_a): single 2-polynomial ciphertexts (stacks are refused); entries of rows that are zero in both
 * LUTs may be 0; at most 8 rows may be used.  nib: n_slots = slot_count bytes, each < 16 (else an error
 * whose message contains "nibble"), copied before the call returns.  The operands are brought to canonical
 * form and dropped exactly to their common lowest logical level l (l < 1: an error containing "level"); the
 * per-slot coefficients are encoded on the device (fp64 FFT codec, no host encode, nothing cached per call)
 * and each output is at level l - 1, owing its rescale as aesfhe_mul_pt_sum's result does.  The per-LUT
 * table D[row][v] is built and uploaded on a LUT's first public evaluation (aesfhe_lut_free releases it);
 * the evaluations themselves never synchronise the stream. */
int aesfhe_lut_eval_public(aesfhe_ctx* ctx, aesfhe_handle lut1, aesfhe_handle lut2 /* 0 = none */,
                           const aesfhe_handle* a, const uint8_t* nib, int n_slots,
                           aesfhe_handle* out1, aesfhe_handle* out2);
/* tests only: the coefficient plaintexts aesfhe_lut_eval_public multiplies by at `level` (>= 1) -- one per
 * used row of `lut` in row order, nl(level) limbs of N words each, NTT form -- and the scale they were
 * encoded at (the level's plaintext scale) */
int aesfhe_debug_public_pt(aesfhe_ctx* ctx, aesfhe_handle lut, const uint8_t* nib, int n_slots, int level, uint32_t* out, double* scale);
/* Releases a LUT's coefficient set and every per-level device constant cached for it (the
 * evaluator's plaintext caches, REF/lut.py:71-94 keeps them per object); fails if `lut` is not
 * a LUT handle.  aesfhe_free also accepts LUT handles; this entry states the intent. */
int aesfhe_lut_free(aesfhe_ctx* ctx, aesfhe_handle lut);
/* Public XOR fused with the value decode: from the Zeta16 nibbles hi, lo of an encrypted byte
 * and PUBLIC nibbles b_hi, b_lo per slot, the real number gain * (16 (hi ^ b_hi) + (lo ^ b_lo)) -- the last XOR
 * of a counter mode (keystream with the public AES ciphertext) and the step from the nibble code to a CKKS
 * number in one plaintext-coefficient sum; no reference counterpart (REF decodes by decrypting).  With
 * zeta = e^(-2 pi i / 16) and a = zeta^k:  val(a ^ b) = sum_{p < 16} E_p[b] a^p,
 * E_p[b] = (1/16) sum_{k < 16} (k ^ b) zeta^(-p k);  E_0 = 7.5, E_8 real, E_(16-p) = conj(E_p), so on codewords
 *     val(a ^ b) = 7.5 + E_8[b] a^8 + T + conj(T),   T = sum_{p = 1..7} E_p[b] a^p.
 * xor_value_create uploads the two 9 x 16 tables (rows E_0..E_8, columns b), hi then lo, row-major re / im
 * ([2][9][16] each), the hi table pre-scaled by 16 gain and the lo table by gain; row 0 is not read (the caller
 * adds the constant gain 7.5 17).  The upload waits for its copy once; xor_value_free (or aesfhe_free) releases it.
 * xor_value_public takes the powers a_hi[p], a_lo[p] = hi^p, lo^p for p = 1..8 (arrays of 9, entry 0 ignored;
 * single 2-polynomial ciphertexts, stacks are refused, a missing one is an error) and the two nibble arrays
 * (n_slots = slot_count bytes each, every byte < 16, else an error containing "nibble"; copied before the call
 * returns), and returns
 *     out_t = sum_{p = 1..7} E_p[b_hi] hi^p + E_p[b_lo] lo^p     (14 ciphertext x plaintext products)
 *     out_r = E_8[b_hi] hi^8 + E_8[b_lo] lo^8                     (2 products, real coefficients)
 * so that out_r + out_t + conj(out_t) + gain 7.5 17 is the value.  The operands are brought to canonical form
 * and dropped exactly to their common lowest logical level l (l < 1: an error containing "level"); the 16
 * per-slot coefficient plaintexts are encoded on the device at the level's plaintext scale (the codec of
 * aesfhe_lut_eval_public, 16 channels at once) and one kernel forms both sums; each output is at level l - 1,
 * owing its rescale as aesfhe_lut_eval_public's outputs do.  A refused call leaves every handle intact; the
 * evaluations never synchronise the stream. */
int aesfhe_xor_value_create(aesfhe_ctx* ctx, const double* re, const double* im, aesfhe_handle* out);
int aesfhe_xor_value_public(aesfhe_ctx* ctx, aesfhe_handle table, const aesfhe_handle* a_hi, const aesfhe_handle* a_lo,
                            const uint8_t* nib_hi, const uint8_t* nib_lo, int n_slots,
                            aesfhe_handle* out_t, aesfhe_handle* out_r);
/* tests only: the 16 coefficient plaintexts aesfhe_xor_value_public multiplies by at `level` (>= 1) -- channel
 * 8 half + (p - 1) holding E_p (p = 1..8) of the hi (half 0) or lo (half 1) table at that half's nibbles,
 * nl(level) limbs of N words each, NTT form -- and the scale they were encoded at */
int aesfhe_debug_xor_value_pt(aesfhe_ctx* ctx, aesfhe_handle table, const uint8_t* nib_hi, const uint8_t* nib_lo, int n_slots, int level,
                              uint32_t* out, double* scale);
/* Typed value decode: aesfhe_xor_value_public with a real WEIGHT and a sign FLAG per slot, for
 * n_groups G = 1 or 2 weight groups over the same operands.  The decoded value is linear in the table, so weight
 * w(s) on every coefficient of slot s gives w(s) * value; a set flag bit 0 makes the hi nibble SIGNED
 * (sval(x) = x - 16 [x >= 8]: the hi table's odd rows negated, since only bit 3 changes weight and bit 3 lives in
 * the odd powers), so 16 sval(hi ^ b_hi) + (lo ^ b_lo) is the two's-complement byte.  `table` is a handle of
 * aesfhe_xor_value_create made from the UNIT tables (16 E and E); the weights carry the gain.
 *   weights: G x n_slots doubles, group-major, all finite (else an error containing "weight not finite"; a null
 *            pointer: "missing weights");  flags: G x n_slots bytes or NULL (no slot signed);
 *   n_groups outside 1..2: an error containing "n_groups".  Everything aesfhe_xor_value_public refuses is refused
 *   with the same words; a refused call leaves every handle intact.
 * Returns G pairs, out_t[g] and out_r[g] (arrays of n_groups handles):
 *     out_t[g] = sum_{p = 1..7} w_g s_p E_p[b_hi] hi^p + w_g E_p[b_lo] lo^p,   out_r[g] = w_g (E_8[b_hi] hi^8 + E_8[b_lo] lo^8)
 * with s_p = -1 on odd p of a flagged slot and 1 elsewhere, so that out_r[g] + out_t[g] + conj(out_t[g]) +
 * w_g (16 c + 7.5) is group g's value (c = -0.5 on a flagged slot, 7.5 elsewhere).  For 16-bit words group g weighs
 * byte g of each word (0 on every other slot) and the caller adds group 1 rotated by the slot distance of the two
 * bytes onto group 0: no mask, no extra level.  One codec pass per group encodes the G x 16 coefficient
 * plaintexts; ONE kernel forms all 2 G sums, reading every ciphertext word once.  Levels, the owed rescale and the
 * copy-before-return rule are aesfhe_xor_value_public's. */
int aesfhe_xor_value_typed(aesfhe_ctx* ctx, aesfhe_handle table, const aesfhe_handle* a_hi, const aesfhe_handle* a_lo,
                           const uint8_t* nib_hi, const uint8_t* nib_lo, int n_slots, int n_groups,
                           const double* weights, const uint8_t* flags, aesfhe_handle* out_t, aesfhe_handle* out_r);
/* tests only: the G x 16 coefficient plaintexts aesfhe_xor_value_typed multiplies by at `level` (>= 1) -- group g's
 * 16 channels (aesfhe_debug_xor_value_pt's order) after group g - 1's -- and the scale they were encoded at */
int aesfhe_debug_xor_value_typed_pt(aesfhe_ctx* ctx, aesfhe_handle table, const uint8_t* nib_hi, const uint8_t* nib_lo, int n_slots,
                                    int n_groups, const double* weights, const uint8_t* flags, int level, uint32_t* out, double* scale);
/* Linear value decode: aesfhe_xor_value_typed for n_groups G = 1..16 weight groups.  With group k
 * weighing the slot of byte position p by W[(p - k) mod 16][p] (the k-th cyclic diagonal of a 16 x 16 matrix W, in
 * slot-position space), sum_k rotate(X_k, k unit) is W applied to the decoded bytes of every state, for no level
 * beyond the decode's own: the caller rotates out_t[k] and out_r[k], adds, and conjugates once.  Arguments, outputs
 * (n_groups handle pairs), levels and refusals are aesfhe_xor_value_typed's, with n_groups outside 1..16 refused
 * ("n_groups").  The groups are walked in chunks of 8: one codec buffer of at most 8 x 16 coefficient plaintexts
 * and ONE kernel per chunk, which reads every ciphertext word once for all of the chunk's sums. */
int aesfhe_xor_value_groups(aesfhe_ctx* ctx, aesfhe_handle table, const aesfhe_handle* a_hi, const aesfhe_handle* a_lo,
                            const uint8_t* nib_hi, const uint8_t* nib_lo, int n_slots, int n_groups,
                            const double* weights, const uint8_t* flags, aesfhe_handle* out_t, aesfhe_handle* out_r);
/* tests only: the G x 16 coefficient plaintexts aesfhe_xor_value_groups multiplies by at `level` (>= 1), in
 * aesfhe_debug_xor_value_typed_pt's order, and the scale they were encoded at */
int aesfhe_debug_xor_value_groups_pt(aesfhe_ctx* ctx, aesfhe_handle table, const uint8_t* nib_hi, const uint8_t* nib_lo, int n_slots,
                                     int n_groups, const double* weights, const uint8_t* flags, int level, uint32_t* out, double* scale);
/* Releases a value table; fails if `table` is not one.  aesfhe_free also accepts value tables. */
int aesfhe_xor_value_free(aesfhe_ctx* ctx, aesfhe_handle table);
/* A 256-entry byte table fused with the value decode.  For a Zeta16 byte (a, c) = (zeta^x_hi,
 * zeta^x_lo) and a public byte b, any real table f satisfies f(x ^ b) = C_00 + T + conj(T) with
 * T = sum_{q = -7..8} y_q U_q, y_q = c^q (q >= 0), conj(c^-q) (q < 0), U_q = sum_{p = 0..8} K_pq[b] a^p.
 * aesfhe_byte_lut_create uploads K -- re / im: [9][16][256] doubles indexed by p, q + 7 and the public byte -- once
 * (it waits for its copy once) and refuses a non-finite entry. */
int aesfhe_byte_lut_create(aesfhe_ctx* ctx, const double* re, const double* im, aesfhe_handle* out);
/* out[q + 7] = U_q = sum_{p = 1..8} weights (.) K_pq[16 nib_hi + nib_lo] (.) a_hi[p] + weights (.) K_0q[16 nib_hi + nib_lo]
 * for q = -7..8: 16 ciphertexts at the operands' common lowest level l, each owing its rescale; the p = 0 column is a
 * per-slot plaintext encoded at the product scale and added inside the sum.  a_hi: 9 handles, the powers hi^p at
 * index p (entry 0 unused); nib_hi / nib_lo: one public nibble (< 16) per slot, n_slots = slot count; weights: one
 * finite real per slot (w = 0 leaves the slot 0).  The 16 groups are walked in chunks of 8: one bounded codec buffer
 * and ONE kernel per chunk, which reads every ciphertext word once for all of the chunk's sums.  Refused with every
 * handle intact: a nibble >= 16 ("nibble"), n_slots != slot count ("slot_count"), operands at level 0 ("level"), a
 * stacked operand ("stack"), a missing power ("used row"), a non-finite or missing weight ("weight"). */
int aesfhe_byte_lut_public(aesfhe_ctx* ctx, aesfhe_handle table, const aesfhe_handle* a_hi, const uint8_t* nib_hi,
                           const uint8_t* nib_lo, int n_slots, const double* weights, aesfhe_handle* out);
/* tests only: the 16 x 9 coefficient plaintexts of aesfhe_byte_lut_public at `level` (>= 1) as [16][9][nl(level)][N]
 * uint32 in NTT form -- group q + 7, then p = 0 (the fill) and p = 1..8 -- and their two scales: scales[0] of the
 * rows p >= 1, scales[1] (the product scale) of the fills */
int aesfhe_debug_byte_lut_pt(aesfhe_ctx* ctx, aesfhe_handle table, const uint8_t* nib_hi, const uint8_t* nib_lo, int n_slots,
                             const double* weights, int level, uint32_t* out, double* scales);
/* Releases a byte table or a bank of them; fails if `table` is not one.  aesfhe_free also accepts byte tables. */
int aesfhe_byte_lut_free(aesfhe_ctx* ctx, aesfhe_handle table);
/* A BANK of byte tables with one table per slot: n_tables coefficient tables K^(0..n_tables-1) of
 * aesfhe_byte_lut_create's layout stored back to back -- re / im: [n_tables][9][16][256] doubles, 1 <= n_tables <= 64
 * (576 KiB of device memory per table, 36 MiB at the cap) -- uploaded once (it waits for its copy once).  Refuses
 * n_tables out of range ("n_tables") and a non-finite entry in any table.  The handle is a byte table handle: a bank
 * of one is what aesfhe_byte_lut_create makes, aesfhe_byte_lut_public on a bank reads its table 0, and
 * aesfhe_byte_lut_free releases it. */
int aesfhe_byte_lut_bank_create(aesfhe_ctx* ctx, const double* re, const double* im, int n_tables, aesfhe_handle* out);
/* aesfhe_byte_lut_public with a table per slot: out[q + 7] = U_q with slot j's coefficients taken from table sel[j] of
 * `bank`, K_pq = K^(sel[j])_pq.  sel: one table index per slot (n_slots bytes), every entry < the bank's n_tables.
 * Operands, outputs, levels and refusals as aesfhe_byte_lut_public's, plus: a missing sel or an entry >= n_tables
 * ("table index"), checked like every other operand before any arithmetic kernel reads it.  One output (its own sel
 * and weights) per call. */
int aesfhe_byte_lut_bank_public(aesfhe_ctx* ctx, aesfhe_handle bank, const aesfhe_handle* a_hi, const uint8_t* nib_hi,
                                const uint8_t* nib_lo, const uint8_t* sel, int n_slots, const double* weights, aesfhe_handle* out);
/* tests only: aesfhe_debug_byte_lut_pt for aesfhe_byte_lut_bank_public (the same row order and scales) */
int aesfhe_debug_byte_lut_bank_pt(aesfhe_ctx* ctx, aesfhe_handle bank, const uint8_t* nib_hi, const uint8_t* nib_lo, const uint8_t* sel,
                                  int n_slots, const double* weights, int level, uint32_t* out, double* scales);
/* Deferred evaluation switch, default on: API-level ct x ct products
 * leave relinearisation and their rescale to the first consumer that needs a
 * 2-polynomial canonical ciphertext (rotate, conjugate, ct x ct, power basis, bootstrap,
 * export), and non-integer scalar / plaintext products defer their rescale.  Sums of such
 * terms are combined before any key switch.  Results decrypt identically up to CKKS
 * rounding; 0 restores eager relinearise-and-rescale after every product. */
int aesfhe_set_lazy(aesfhe_ctx* ctx, int on);
/* engine.relinearize, REF/engine_context.py:134-145 */
int aesfhe_relinearize(aesfhe_ctx* ctx, aesfhe_handle ct, aesfhe_handle* out);
int aesfhe_rescale(aesfhe_ctx* ctx, aesfhe_handle ct, aesfhe_handle* out);
/* drop to a lower level with exact scale */
int aesfhe_level_down(aesfhe_ctx* ctx, aesfhe_handle ct, int level, aesfhe_handle* out);
/* engine.rotate(ct, rotation_key, steps), REF/engine_context.py:127-132 */
int aesfhe_rotate(aesfhe_ctx* ctx, aesfhe_handle ct, int steps, aesfhe_handle* out);
/* engine.conjugate(ct, conjugation_key), REF/engine_context.py:103-104 */
int aesfhe_conjugate(aesfhe_ctx* ctx, aesfhe_handle ct, aesfhe_handle* out);
/* Batched variants (SURVEY.md §8(b) "optional batched variants taking h[] arrays"; DESIGN.md
 * §3.12): n independent engine.multiply(a[i], b[i], relinearization_key) products
 * (REF/engine_context.py:65-67, always relinearised and rescaled) resp. n
 * engine.conjugate(in[i], conjugation_key) calls (REF/engine_context.py:103-104).  Operands
 * at one level are stacked and share one tensor launch and one key switch per chunk of four;
 * the results equal the separate calls bit for bit.  out[i] receives a new handle. */
int aesfhe_mul_many(aesfhe_ctx* ctx, int n, const aesfhe_handle* a, const aesfhe_handle* b, aesfhe_handle* out);
/* sum_{i<n} cts[i] * pts[i] (1 <= n <= 8 single ciphertexts times non-constant plaintexts), at the
 * operands' common lowest level, as ONE kernel; the same value as n engine.multiply(ct, pt) calls summed
 * with engine.add (REF/engine_context.py:65-68, :77-80) -- the masked rotations of REF/shift_rows.py:39-56
 * feeding MixColumns (REF/mixcol_final.py:124-154) summed in one launch (MixColFinal.sr_entry). */
int aesfhe_mul_pt_sum(aesfhe_ctx* ctx, int n, const aesfhe_handle* cts, const aesfhe_handle* pts, aesfhe_handle* out);
/* the secret-key renorm's pool of zero encryptions: size = encryptions made per
 * refill (0: every renorm encrypts its own message; < 0: keep the size), every pool emptied -- the
 * re-encryption of REF/pipeline.py:65-69 (decrypt -> snap -> encrypt) drawn as Enc(0) + message */
int aesfhe_renorm_pool(aesfhe_ctx* ctx, int size);
/* members per packed bootstrap of a stacked periodic ciphertext (aesfhe_bootstrap_sparse on a stack):
 * up to `members` (a power of two dividing the stack size) monomial-packed into one message of
 * `members` times the period, one bootstrap each.  1: every member its own
 * bootstrap (bit-exact with single bootstraps); default 16 (AESFHE_STACK_PACK). */
int aesfhe_set_stack_pack(aesfhe_ctx* ctx, int members);
int aesfhe_conjugate_many(aesfhe_ctx* ctx, int n, const aesfhe_handle* in, aesfhe_handle* out);
/* n automorphisms of possibly DIFFERENT ciphertexts, each with its own Galois element galois[i]
 * (odd, < 2N): engine.rotate(ct, rotation_key, steps) (REF/engine_context.py:127-132; Galois
 * element 5^(-steps) mod 2N) and engine.conjugate(ct, conjugation_key) (:103-104; 2N - 1) calls
 * of one AES step -- the masked row rotations of ShiftRows (REF/shift_rows.py:39-56) and the
 * column shifts of MixColumns (REF/mixcol_final.py:124-154) for both nibble halves -- as ONE
 * heterogeneous batched key switch per level: one ModUp per distinct input,
 * one key-inner-product launch with a key per member, one stacked ModDown.  Same results as the
 * separate calls; galois[i] = 1 returns a copy. */
int aesfhe_galois_multi(aesfhe_ctx* ctx, int n, const aesfhe_handle* in, const uint64_t* galois, aesfhe_handle* out);

/* Stacked ciphertexts (multi-pair batches, BASELINE configs 3-5 with one state per pair; DESIGN.md
 * §3.16).  aesfhe_stack: n single ciphertexts -> ONE handle holding n members (canonical form,
 * dropped to the lowest member level).  Every operation then takes the stack as one operand and
 * returns a stack: element-wise work in one launch over all members, key switches in chunks of
 * members that read each key once, LUT sums with a member grid dimension, renorms decrypting /
 * re-encrypting every member in one set of launches, bootstraps in chunks of two members.
 * Operands of one operation must be stacks of the same size (no broadcasting); decrypt needs a
 * single ciphertext.  aesfhe_unstack: the n members as single handles (n = member count);
 * aesfhe_members: the member count (1 for a single ciphertext).  Replaces the reference's loop
 * over independent ciphertext pairs (REF/main.py:121-140 runs one pair per state). */
int aesfhe_stack(aesfhe_ctx* ctx, int n, const aesfhe_handle* in, aesfhe_handle* out);
int aesfhe_unstack(aesfhe_ctx* ctx, aesfhe_handle in, int n, aesfhe_handle* out);
int aesfhe_members(aesfhe_ctx* ctx, aesfhe_handle h, int* members);
/* n rotations of ONE ciphertext, engine.rotate(ct, rotation_key, steps[i])
 * (REF/engine_context.py:127-132; the column shifts of REF/mixcol_final.py:124-154 and the
 * row rotations of REF/shift_rows.py:39-56), hoisted: one ModUp for all of them.  Same
 * results as n aesfhe_rotate calls. */
int aesfhe_rotate_hoisted(aesfhe_ctx* ctx, aesfhe_handle ct, int n, const int* steps, aesfhe_handle* out);
/* Masked rotation sum of ONE ciphertext, double-hoisted:
 *   out[j] = sum_i pts[j*n + i] * rotate(ct, steps[i]),  j < n_out (1..2), i < n (1..16);
 * pts entries may be 0 (term absent); steps[i] may be 0 (no key switch for that term).  The same value as
 * n aesfhe_rotate calls, aesfhe_mul_pt each and aesfhe_add (REF/engine_context.py:127-132, :65-68, :70-74;
 * the masked rotations of REF/shift_rows.py:39-56 generalised to a permutation inside the state's columns,
 * shift_columns.py), within CKKS rounding and not bit-exact: c1 is ModUp'ed once, every used rotation's key
 * inner product is multiplied by its mask and summed in Q*P, and each output pays ONE ModDown (after the
 * mask instead of before it).  rotate keeps np.roll's convention.  The input is brought to canonical form;
 * each output is at that level and owes its rescale as aesfhe_mul_pt_sum's result does.  It runs over the
 * level's own special basis (aesfhe_set_low_p on or off); the masks are encoded once per (plaintext, level,
 * special-prime count) over those limbs, cached on the plaintext handle and released with it.  Stacks and
 * 3-polynomial inputs are refused. */
int aesfhe_rot_pt_sum(aesfhe_ctx* ctx, aesfhe_handle ct, int n, const int* steps, int n_out, const aesfhe_handle* pts,
                      aesfhe_handle* out);
/* The affine form of aesfhe_rot_pt_sum (the homomorphic AES key schedule, key_expansion.py):
 *   out[j] = sum_i pts[j*n + i] * rotate(ct, steps[i]) + fills[j],  j < n_out;
 * fills holds n_out plaintext handles, 0 = no fill for that output.  Slots no mask covers come out as the
 * fill's value instead of 0 (which is no Zeta16 codeword).  aesfhe_rot_pt_sum's contract in every other
 * respect: canonical input, one ModUp, one kernel, one ModDown per output, the level's own special basis with
 * aesfhe_set_low_p on or off, outputs owing their rescale, the same refusals.  A fill is encoded at the
 * product scale (the raw scale of an output that owes its rescale) over the output's limbs, cached on its
 * handle per (level, special-prime count) and released with it, and added inside the sum's kernel.  With
 * every fill 0 the outputs equal aesfhe_rot_pt_sum's bit for bit. */
int aesfhe_rot_pt_affine(aesfhe_ctx* ctx, aesfhe_handle ct, int n, const int* steps, int n_out, const aesfhe_handle* pts,
                         const aesfhe_handle* fills, aesfhe_handle* out);
/* engine.make_power_basis(ct, degree, relinearization_key), REF/engine_context.py:100-101;
 * out[k-1] = ct^k, k = 1..degree */
int aesfhe_power_basis(aesfhe_ctx* ctx, aesfhe_handle ct, int degree, aesfhe_handle* out);
/* engine.ntt / engine.intt, REF/engine_context.py:173-177 */
int aesfhe_to_ntt(aesfhe_ctx* ctx, aesfhe_handle ct, aesfhe_handle* out);
int aesfhe_to_intt(aesfhe_ctx* ctx, aesfhe_handle ct, aesfhe_handle* out);
/* engine.bootstrap(ct, relin, conj, bootstrap_key), REF/engine_context.py:147-162.
 * Full-slot complex bootstrapping: sparse-secret encapsulation, ModRaise,
 * CoeffToSlot, EvalMod, SlotToCoeff.  Input slots must satisfy |z| <= 1; the output is at
 * level max_level - aesfhe_bootstrap_depth() of the bootstrappable parameter set. */
int aesfhe_bootstrap(aesfhe_ctx* ctx, aesfhe_handle ct, aesfhe_handle* out);
/* the two bootstraps of a hi / lo pair (REF/mixcol_final.py:158-162, REF/invmixcolumns_fhe.py:166-168)
 * as one batched bootstrap: same results as two aesfhe_bootstrap calls, each key switch reads
 * its key and each linear transform its diagonals once for both */
int aesfhe_bootstrap_pair(aesfhe_ctx* ctx, aesfhe_handle a, aesfhe_handle b, aesfhe_handle* out_a, aesfhe_handle* out_b);
/* bootstrap(ct) * gain and its pair form, gain in (0, 1] folded into the level-0 scaling (no
 * extra level): the true-FHE renorm's bootstrap hands the snap u = kappa x (REF
 * zeta16_noise_reducter.py:6-57 bootstrap_before=True) */
int aesfhe_bootstrap_scaled(aesfhe_ctx* ctx, aesfhe_handle ct, double gain, aesfhe_handle* out);
/* Sparse-slot bootstrap: for a message whose slots repeat with period `period`
 * (slot j == slot j mod period; a power of two in [16, slot_count)), i.e. a polynomial in the
 * subring Z[X^(N / 2 period)].  Same result as aesfhe_bootstrap on such a message (within the
 * bootstrap's error) at a fraction of the cost: a trace to the subring after ModRaise, then the
 * period-sized CoeffToSlot / SlotToCoeff; it starts from a lower level.  A message that is not
 * periodic is NOT refreshed correctly.  gain as for aesfhe_bootstrap_scaled (1.0 = none).
 * Replaces the same engine.bootstrap calls (REF/engine_context.py:147-162) when the caller
 * knows its layout is periodic (StateEncoder(periodic=True)). */
int aesfhe_bootstrap_sparse(aesfhe_ctx* ctx, aesfhe_handle ct, int period, double gain, aesfhe_handle* out);
/* Secret-key renorm of a (hi, lo) pair in the periodic layout (slot j == slot j mod period,
 * a power of two >= 16): period 16 decodes / re-encodes its 16 slots directly, other periods
 * snap every slot; level < 0 = the fresh level (as aesfhe_renorm_at otherwise). */
int aesfhe_renorm_periodic(aesfhe_ctx* ctx, aesfhe_handle hi, aesfhe_handle lo, int period, int level, aesfhe_handle* out_hi,
                           aesfhe_handle* out_lo);
/* Secret-key renorm of ONE ciphertext whose every slot holds a Zeta16 nibble (a packed state
 * of the pipeline's packed XOR stage): every slot snapped and re-encrypted at
 * `level` (< 0 = fresh).  Replaces the renorm of REF/pipeline.py:65-69 for that form. */
int aesfhe_renorm_single(aesfhe_ctx* ctx, aesfhe_handle ct, int level, aesfhe_handle* out);
/* aesfhe_renorm_single of a ciphertext known to be `period`-periodic (the packed form: period =
 * 2 x the state period): period 32 decodes / re-encodes its 32 slots directly (no FFT); other
 * periods as aesfhe_renorm_single. */
int aesfhe_renorm_packed(aesfhe_ctx* ctx, aesfhe_handle ct, int period, int level, aesfhe_handle* out);
/* Secret-key renorm that unpacks: `packed` holds the hi nibbles of an n-periodic state pair in
 * slots (j mod 2n) < n and the lo nibbles in the others (period = n, a power of two, 2n <=
 * slots); out_hi / out_lo are the snapped n-periodic hi / lo states at `level` -- the
 * (hi, lo) pair REF/pipeline.py:65-69's renorm returns. */
int aesfhe_renorm_unpack(aesfhe_ctx* ctx, aesfhe_handle packed, int period, int level, aesfhe_handle* out_hi,
                         aesfhe_handle* out_lo);
/* aesfhe_renorm_periodic / _packed / _unpack of ct + conj(ct_conj) (per channel for the pair): a conjugate-split LUT's S1 + conj(S2)
 * renormalised without its conjugation key switch (both decrypted, conj(m2) = m2(X^-1) added before
 * the codec); inputs of different level / scale are summed homomorphically first.  Engine-side
 * fusion of REF's `ctx.add(s1, ctx.conjugate(s2))` followed by the renorm (REF/pipeline.py:65-69). */
/* the periodic pair renorm (period 16, one state pair) whose output is ONE ciphertext in the packed
 * period-32 form (hi on slots j mod 32 < 16, lo on the others: StateEncoder.pack's layout) -- the
 * renorm of pack(hi, lo) without the pack's mask products and level; hi_conj / lo_conj (both or
 * neither, 0 = none): the pair's conjugate partners as aesfhe_renorm_periodic_conj. */
/* the periodic pair renorm (period 16, one state pair) with a byte permutation folded in: output slot
 * i (byte i) takes input byte perm16[i] (ShiftRows: REF/shift_rows.py's slot rotations after the renorm
 * of REF/pipeline.py:65-69, at no level); optional conjugate partners as aesfhe_renorm_periodic_conj;
 * pack_out != 0: one packed output as aesfhe_renorm_pack (out_lo unused). */
int aesfhe_renorm_periodic_perm(aesfhe_ctx* ctx, aesfhe_handle hi, aesfhe_handle lo, aesfhe_handle hi_conj, aesfhe_handle lo_conj,
                                const int32_t* perm16, int pack_out, int period, int level, aesfhe_handle* out_hi, aesfhe_handle* out_lo);
/* aesfhe_renorm_unpack (period 16) with a byte permutation folded in, applied to both unpacked
 * halves (InvShiftRows after the renorm that follows InvMixColumns); packed_conj: 0 or a conjugate partner */
int aesfhe_renorm_unpack_perm(aesfhe_ctx* ctx, aesfhe_handle packed, aesfhe_handle packed_conj, const int32_t* perm16, int period, int level,
                              aesfhe_handle* out_hi, aesfhe_handle* out_lo);
int aesfhe_renorm_pack(aesfhe_ctx* ctx, aesfhe_handle hi, aesfhe_handle lo, aesfhe_handle hi_conj, aesfhe_handle lo_conj, int period, int level,
                       aesfhe_handle* out);
int aesfhe_renorm_periodic_conj(aesfhe_ctx* ctx, aesfhe_handle hi, aesfhe_handle lo, aesfhe_handle hi_conj, aesfhe_handle lo_conj,
                                int period, int level, aesfhe_handle* out_hi, aesfhe_handle* out_lo);
int aesfhe_renorm_packed_conj(aesfhe_ctx* ctx, aesfhe_handle ct, aesfhe_handle ct_conj, int period, int level, aesfhe_handle* out);
int aesfhe_renorm_unpack_conj(aesfhe_ctx* ctx, aesfhe_handle packed, aesfhe_handle packed_conj, int period, int level,
                              aesfhe_handle* out_hi, aesfhe_handle* out_lo);
int aesfhe_bootstrap_pair_sparse(aesfhe_ctx* ctx, aesfhe_handle a, aesfhe_handle b, int period, double gain, aesfhe_handle* out_a,
                                 aesfhe_handle* out_b);
int aesfhe_bootstrap_pair_scaled(aesfhe_ctx* ctx, aesfhe_handle a, aesfhe_handle b, double gain, aesfhe_handle* out_a,
                                 aesfhe_handle* out_b);
/* four n-periodic ciphertexts (4 period <= slots) refreshed by ONE bootstrap at period 4n: the pairs
 * (in[0], in[1]) and (in[2], in[3]) monomial-packed as in aesfhe_bootstrap_pair_sparse, the two packs
 * packed once more (X^(N/8n)), split back by rotations by 2n then n slots.  out[m] = gain * in[m]
 * refreshed (the true-FHE MixColumns renorms of two ciphertext pairs at one point of a round;
 * replaces two aesfhe_bootstrap_pair_sparse calls, REF/zeta16_noise_reducter.py:108-169 /
 * REF/mixcol_final.py:104-106's renorm points). */
int aesfhe_bootstrap_quad_sparse(aesfhe_ctx* ctx, const aesfhe_handle* in, int period, double gain, aesfhe_handle* out);
int aesfhe_bootstrap_depth(void);
/* host self-check of the bootstrap plan: err[0] SlotToCoeff, err[1] CoeffToSlot vs the
 * canonical embedding, err[2] EvalMod Chebyshev error (no GPU needed) */
int aesfhe_debug_bootplan(int log_n, double* err3);
/* the same self-check for a sparse (period-n) plan, packed real form or not: err2 = [StC, CtS] */
int aesfhe_debug_sparseplan(int n, int pack, double* err2);
/* debug: run bootstrap up to a stage (1..11, see engine.hip) and return that ciphertext */
int aesfhe_debug_boot_stage(aesfhe_ctx* ctx, aesfhe_handle ct, int stage, aesfhe_handle* out);
/* Sparse-slot bootstrap stages and groups (tests only, no reference counterpart:
 * the pieces of the bootstrap that replaces engine.bootstrap at REF/mixcol_final.py:158-162).
 * debug_boot_stage_sparse: the period-`period` bootstrap stopped after a stage (as
 * aesfhe_debug_boot_stage; 12 = back on the dense secret BEFORE the trace to the subring, 4 =
 * after it, 9 = the packed real form w' + conj(w'), 10 = after EvalMod).  debug_sparse_group:
 * one CoeffToSlot (which < #CtS) / SlotToCoeff group of that plan (pair != 0: the pair-packed
 * plan; its last index is the lo form of SlotToCoeff's first group); debug_sparse_group_plain:
 * the same group on the host on the first info3[0] slots (one period of its diagonals), tiled
 * over all slot_count outputs; info3[1] = CoeffToSlot groups, info3[2] = all groups.  debug_mono_pack: a + X^(N / 4 period) b at level 0;
 * debug_mono_split: (m + rot_period(m), X^-k (m - rot_period(m))) -- the monomial pair packing
 * and its split around ONE bootstrap of both messages. */
int aesfhe_debug_boot_stage_sparse(aesfhe_ctx* ctx, aesfhe_handle ct, int stage, int period, aesfhe_handle* out);
int aesfhe_debug_sparse_group(aesfhe_ctx* ctx, aesfhe_handle ct, int period, int which, int pair, aesfhe_handle* out);
int aesfhe_debug_sparse_group_plain(aesfhe_ctx* ctx, int period, int which, int pair, const double* re, const double* im,
                                    double* out_re, double* out_im, int* info3);
int aesfhe_debug_mono_pack(aesfhe_ctx* ctx, aesfhe_handle a, aesfhe_handle b, int period, aesfhe_handle* out);
int aesfhe_debug_mono_split(aesfhe_ctx* ctx, aesfhe_handle m, int period, aesfhe_handle* out_hi, aesfhe_handle* out_lo);
/* Result pack: 1 <= n_members <= 32 single ciphertexts (no stacks), at any levels and in any
 * deferred state, as ONE ordinary level-0, two-polynomial, NTT-form ciphertext at scale delta_0:
 *   z = sum_j X^(j k') ct_j,  k' = N / (2 period G),  G = the smallest power of two >= n_members,
 * a G period-periodic message.  Each member must be `period`-periodic (slot j == slot j mod period): the caller's
 * assertion, exactly as for aesfhe_renorm_periodic -- a member that is not is packed wrongly, without an error.  A
 * handle of 0 is an absent member and contributes zero.  period: a power of two >= 1 with G period <= slot_count.
 * Every member is brought to canonical form and dropped exactly to level 0; the pack is a sum of monomial products,
 * so it takes no key switch and no level and adds only the members' own noise, and it runs on an evaluation-only
 * context.  Convention: two members give aesfhe_debug_mono_pack's words; four members [a, c, b, d] give those of
 * mono_pack(mono_pack(a, b, period), mono_pack(c, d, period), 2 period).  The holder of the secret decrypts once and
 * separates the members in the clear (result_pack.split_slots).  Refused (status -1, aesfhe_last_error; nothing is
 * kept, the context stays usable): n_members outside 1..32, every member absent, a stack as a member, a period that
 * is no power of two, G period > slot_count. */
int aesfhe_pack_periodic(aesfhe_ctx* ctx, int n_members, const aesfhe_handle* members, int period, aesfhe_handle* out);
/* Ring switch: ONE single ciphertext (no stack), at any level and in any deferred state, whose
 * message lies in the subring Z[X^k], k = N / ring -- the caller's assertion, exactly as periodicity is for
 * aesfhe_pack_periodic (a result pack with 2 G period <= ring is such a message); a message outside the subring is
 * switched wrongly, without an error.  The ciphertext is brought to canonical two-polynomial form and to level 0 as
 * aesfhe_pack_periodic brings its members, key-switched to the subring secret s_R (a uniform ternary polynomial of
 * Z[X^k]) over Q0 P' and decimated: out is [2][2][ring] uint32, the COEFFICIENT-form residues mod q0 and q1, below
 * their moduli, of (c0', c1') at coefficient indices 0, k, 2k, ..., which decrypt as c0' + c1' s_R in
 * Z[X] / (X^ring + 1) at scale delta_0.  ring: a power of two below N.  Security gate: the ring key splits into k RLWE
 * samples of dimension `ring` at modulus Q0 P' (the key has two digits, q0 and q1, so one special prime suffices;
 * layout [2][2][2 + np][N], tag 12 N + ring), so P' is the largest prefix of the dense -> sparse key's special
 * primes with log2(Q0 P') within the HE standard's bound for `ring` (ternary secret, 128 bits classical: 27 / 54 /
 * 109 / 218 / 438 / 881 for 1024 .. 32768); a ring below 1024 or one that admits not even one special prime is
 * refused with "ring too small for this modulus" unless insecure_ok != 0, which exists for small test rings only.
 * Refused before the first launch (status -1, aesfhe_last_error; nothing is kept, the context stays usable): a ring
 * that is no power of two or >= N, words < 4 ring, a stack as input, a ring the gate rejects.  A keyed context makes
 * the ring key on first use; an evaluation-only context without it fails with "evaluation key missing".
 * aesfhe_ensure_ring_key: the key alone, under the same gate (the client's warm-up before it exports its keys;
 * aesfhe_ensure_key with the key's tag does the same without insecure_ok).  aesfhe_export_ring_secret: the `ring`
 * ternary coefficients of s_R (its coefficients at 0, k, 2k, ...), keyed contexts only ("no secret key" otherwise). */
int aesfhe_ring_switch(aesfhe_ctx* ctx, aesfhe_handle ct, int ring, int insecure_ok, uint32_t* out, uint64_t words);
int aesfhe_ensure_ring_key(aesfhe_ctx* ctx, int ring, int insecure_ok);
int aesfhe_export_ring_secret(aesfhe_ctx* ctx, int ring, int32_t* out);
/* ephemeral sparse secret (NTT form, all limbs) */
int aesfhe_export_sparse(aesfhe_ctx* ctx, uint32_t* out);
int aesfhe_debug_lin_group(aesfhe_ctx* ctx, aesfhe_handle ct, int which, aesfhe_handle* out);
/* The same group applied on the host to slot_count complex slots (re, im) -> (out_re, out_im):
 * the plan model a decryption of aesfhe_debug_lin_group is checked against (test only). */
int aesfhe_debug_lin_group_plain(aesfhe_ctx* ctx, int which, const double* re, const double* im, double* out_re,
                                 double* out_im);
/* [s_bt, k1, top, K, r, deg, log2 modulus of the dense->sparse key (Q0 P', Q0 = q0 q1), sparse
 * secret weight h, special primes in P', base limbs in Q0, message bits b (s_bt = Q0 / 2^b)]
 *  */
int aesfhe_boot_info(aesfhe_ctx* ctx, double* out11);
/* Zeta16 secret-key renorm of a (hi, lo) state pair (REF/pipeline.py:65-69): decrypt,
 * snap the 16 strided slots to the nearest codeword, refill others with 1, re-encrypt */
int aesfhe_renorm_pair(aesfhe_ctx* ctx, aesfhe_handle hi, aesfhe_handle lo, aesfhe_handle* out_hi, aesfhe_handle* out_lo);
/* the same renorm for the slot-packed layout: `states` AES states per
 * ciphertext pair, byte i of state b in slot i*stride + b (1 <= states <= slot_count/16);
 * every slot with (j mod stride) < states is snapped, the others refilled with 1.
 * Replaces the per-state loop over REF/pipeline.py:65-69 for a batch of states. */
int aesfhe_renorm_states(aesfhe_ctx* ctx, aesfhe_handle hi, aesfhe_handle lo, int states, aesfhe_handle* out_hi,
                         aesfhe_handle* out_lo);
/* renorm_states re-encrypting at min(level, fresh) (< 0 = the fresh level) instead of the
 * fresh level: a caller that knows the depth of its next step saves limbs */
int aesfhe_renorm_at(aesfhe_ctx* ctx, aesfhe_handle hi, aesfhe_handle lo, int states, int level, aesfhe_handle* out_hi,
                     aesfhe_handle* out_lo);

/* --- raw access (tests, parity against the oracle) ------------------------------------ */
/* limbs of a ciphertext: npoly x (level+2) x N uint32, NTT form */
int aesfhe_export(aesfhe_ctx* ctx, aesfhe_handle ct, uint32_t* out, uint64_t words);
int aesfhe_import(aesfhe_ctx* ctx, int level, int npoly, const uint32_t* data, aesfhe_handle* out);
/* secret key (NTT form, all n_q + n_p limbs) / public key / key-switching key of galois g (0 = relin) */
int aesfhe_export_secret(aesfhe_ctx* ctx, uint32_t* out);
int aesfhe_export_pk(aesfhe_ctx* ctx, uint32_t* out);
int aesfhe_export_ksk(aesfhe_ctx* ctx, uint64_t galois, uint32_t* out);
/* the key a key switch of galois g at `level` runs with: on a reduced level (aesfhe_set_low_p, nl = level's limbs
 * < alpha) that level's own single-digit key, [2][nl + np][N] with np = nl + 1 (Q limbs 0..nl-1, then the first np
 * special primes); on any other level the full key, as aesfhe_export_ksk */
int aesfhe_export_ksk_at(aesfhe_ctx* ctx, uint64_t galois, int level, uint32_t* out);
/* forward / inverse NTT of host rows whose limb l is prime first_prime + l */
int aesfhe_debug_ntt(aesfhe_ctx* ctx, uint32_t* data, int rows, int first_prime, int inverse);
/* key switch of a raw polynomial d (level+2 limbs, NTT) with the key of galois g */
int aesfhe_debug_keyswitch(aesfhe_ctx* ctx, int level, uint64_t galois, const uint32_t* d, uint32_t* out);
/* per-kernel timing of the last N ops (HIP events); op counters */
/* Micro-benchmark of one primitive, iters back-to-back launches on the engine stream;
 * *us = microseconds per iteration (device time incl. launch gaps).  op 0: NTT of arg
 * rows, 1: inverse NTT of arg rows, 2: key switch at level arg, 3: rescale at level arg,
 * 4: ct x ct + relinearise + rescale at level arg.  MI355X-side tooling. */
int aesfhe_bench_op(aesfhe_ctx* ctx, int op, int arg, int iters, double* us);
int aesfhe_counters(aesfhe_ctx* ctx, uint64_t* out, int n);
/* time only one launch in `every` of each enabled kernel (default 1): an unbiased live sample
 * with less event overhead in the measured run */
int aesfhe_profile_every(aesfhe_ctx* ctx, int every);
/* live kernel timing with HIP events on the engine stream: bit k of mask enables kernel id k
 * (order: ntt_cols_fwd, ntt_rows_fwd, ntt_rows_inv, ntt_cols_inv, base_convert, key_inner,
 * moddown, tensor, rescale, automorph, elementwise, sample); stats: per id
 * [launches, total ms, algorithmic bytes] */
int aesfhe_profile(aesfhe_ctx* ctx, uint32_t mask);
int aesfhe_kernel_stats(aesfhe_ctx* ctx, double* out, int n, int reset);
/* radix-2 butterflies of the timed NTT launches per kernel id (out[n]; call before a resetting
 * aesfhe_kernel_stats): the numerator of the NTT's VALU roofline */
int aesfhe_kernel_work(aesfhe_ctx* ctx, double* out, int n);
/* dispatch-inclusive timing: per kernel id k, out[2k] = boundary gaps measured, out[2k + 1] = their
 * total ms -- the gap between the last block end of a sampled launch and the first block start of
 * the launch issued right after it, accounted to the latter's id (its drain + dispatch ramp, what
 * rocprofv3 durations add to the in-kernel span); call before a resetting aesfhe_kernel_stats */
int aesfhe_kernel_gaps(aesfhe_ctx* ctx, double* out, int n);
/* per-level work tallies since the last aesfhe_reset_counters: out[l] (l < n) = kind 0 key switches
 * of one polynomial (hoisted rotations counted one each), 1 ct x ct products (tensor + relinearise +
 * rescale; their key switch counted in kind 0), 2 plaintext-diagonal products of the linear transforms,
 * at level l.  The CPU baseline replays a bootstrap's work from them on the C oracle (bench.py). */
int aesfhe_level_counters(aesfhe_ctx* ctx, int kind, uint64_t* out, int n);
int aesfhe_reset_counters(aesfhe_ctx* ctx);
/* device memory pool: out[0] = bytes the context's buffer pools hold (in use + cached), out[1] =
 * allocations that failed, released the cached free lists and were retried (a second failure is
 * an error status).  AESFHE_POOL_LIMIT_MB caps the pool bytes (test switch) */
int aesfhe_pool_stats(aesfhe_ctx* ctx, uint64_t* out);
/* kernel launches issued by this process so far (all contexts): the launch census of
 * tools/launch_census.py and bench.py's launches-per-encrypt (MI355X-side tooling) */
uint64_t aesfhe_launch_count(void);
/* launch census by (C-ABI entry point, kernel name), collected when the process starts with
 * AESFHE_CENSUS=1: "entry\tkernel\tlaunches\n" lines into buf (NUL-terminated, truncated to cap);
 * returns the bytes the whole census needs; reset != 0 clears it (tools/op_kernel_census.py) */
uint64_t aesfhe_launch_census(char* buf, uint64_t cap, int reset);
/* per kernel id (the aesfhe_profile order): algorithmic bytes and launches of
 * every launch this process issued so far, timed or not -- bench.py's whole-step roofline
 * (sum of algorithmic bytes of the timed steps / wall / 8 TB/s) */
int aesfhe_alg_bytes(double* bytes, uint64_t* launches, int n);

#ifdef __cplusplus
}
#endif
#endif
