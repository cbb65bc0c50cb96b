"""GPU: every GEMM kernel variant, bit for bit, on operands for which fp32 arithmetic is exact.

Entries of A, B, the bias and the prior contents of C are non-zero integers in [-a, a], a <= 8 chosen per case so that
2 K a^2 + 2 a < 2^24.  Every partial sum, in every order, is then an integer below 2^24: every fma, every MFMA step and every
fp32 atomic add is exact, and so are bias + product and C + product.  Integers up to 256 are exact in bfloat16, so the bf16
families round nothing, and the three-piece split of gemm_x3.hip puts such a value whole into its first piece.  A correct kernel
therefore returns the bits of the integer product -- whatever its tile, its K cut, its atomics or its order of accumulation --
and one dropped, doubled or misplaced term changes an element by at least 1.  The reference is torch's float64 product (exact for
these values), never another entry point of the library; every comparison is torch.equal.  There is no tolerance in this file.

Every output sits inside a larger buffer: guard rows before and after, guard columns when ldc > N, all holding 777.0 (a stray
store, add or atomic of a non-zero integer changes it); every guard element must keep its bits.  The logical block starts as NaN
(accumulate 0: the clear pass of a cut product and the "C need not be cleared" promise of the ordered calls), as random integers
(accumulate 1) or as zeros (accumulate 2).  Operands sit in NaN-filled buffers, padding columns included: an element read from
outside a matrix shows in the result.

CASES has one row per intended kernel variant: the call, then what the row is meant to REACH -- tile BM x BN, predicate-free
(FAST) or predicated (PRED) kernel, K slices -- and the reason for the row.  The slice count and BM are asserted from the
library's queries (check_claims, also run without a GPU by tests/test_gemm_variants_host.py); BN and FAST / PRED cannot be
queried: they are derived by hand from gemm_plan, gemm_bf16_plan and the families' fast().  tests/test_gemm_variants_host.py
compares the set of (family, BM, BN, transposes, FAST) the rows claim with the gemm_f32_kernel / gemm_bf16_kernel
instantiations in the built library: a new tile shape or kernel variant needs a row here before that test passes again."""
import collections
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FAST, PRED = True, False
Case = collections.namedtuple("Case", "id entry fam ta tb M N K BM BN fast slices why opts")


def C(id, entry, fam, ta, tb, M, N, K, BM, BN, fast, slices, why, **opts):
    return Case(id, entry, fam, ta, tb, M, N, K, BM, BN, fast, slices, why, opts)


# waves per workgroup side of every tile shape (the WM, WN template arguments next to BM, BN)
WAVES = {(32, 128): (1, 4), (64, 64): (2, 2), (128, 160): (4, 1), (160, 128): (1, 4), (128, 64): (4, 1), (64, 128): (2, 2),
         (128, 128): (2, 2)}

# id, entry, family, trans_a, trans_b, M, N, K | reaches: BM, BN, FAST / PRED, K slices | why | options:
#   acc = accumulate modes run (default (0,)); bias (default: yes where the entry takes one);
#   lda_extra / ldb_extra / ldc_extra = floats added to the leading dimension (which is otherwise the width rounded up to 4);
#   a_off / b_off = floats the operand's base is moved off its 16-byte alignment; fold_b / fold_c = fold widths.
# A predicated row states the ONE reason it leaves the predicate-free kernel where the plan rules allow a single reason (a 160-wide
# tile has no ragged 160 side: its rule asks for a multiple of 160).
CASES = [
    # f32 32x128
    C("f32-32x128-whole-00", "gemm", "f32", 0, 0, 32, 128, 64, 32, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("f32-32x128-whole-01", "gemm", "f32", 0, 1, 32, 128, 64, 32, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("f32-32x128-whole-10", "gemm", "f32", 1, 0, 32, 128, 64, 32, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("f32-32x128-whole-11", "gemm", "f32", 1, 1, 32, 128, 64, 32, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("f32-32x128-m1-00", "gemm", "f32", 0, 0, 1, 128, 64, 32, 128, PRED, 1, "one row", acc=(0, 1)),
    C("f32-32x128-m1-01", "gemm", "f32", 0, 1, 1, 128, 64, 32, 128, PRED, 1, "one row", acc=(0, 1)),
    C("f32-32x128-m1-10", "gemm", "f32", 1, 0, 1, 128, 64, 32, 128, PRED, 1, "one row", acc=(0, 1)),
    C("f32-32x128-m1-11", "gemm", "f32", 1, 1, 1, 128, 64, 32, 128, PRED, 1, "one row", acc=(0, 1)),
    C("f32-32x128-ragN-00", "gemm", "f32", 0, 0, 32, 130, 64, 32, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-32x128-ragN-01", "gemm", "f32", 0, 1, 32, 130, 64, 32, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-32x128-ragN-10", "gemm", "f32", 1, 0, 32, 130, 64, 32, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-32x128-ragN-11", "gemm", "f32", 1, 1, 32, 130, 64, 32, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-32x128-ragK-00", "gemm", "f32", 0, 0, 32, 128, 70, 32, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-32x128-ragK-01", "gemm", "f32", 0, 1, 32, 128, 70, 32, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-32x128-ragK-10", "gemm", "f32", 1, 0, 32, 128, 70, 32, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-32x128-ragK-11", "gemm", "f32", 1, 1, 32, 128, 70, 32, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-32x128-ragMNK-00", "gemm", "f32", 0, 0, 17, 130, 70, 32, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-32x128-ragMNK-01", "gemm", "f32", 0, 1, 17, 130, 70, 32, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-32x128-ragMNK-10", "gemm", "f32", 1, 0, 17, 130, 70, 32, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-32x128-ragMNK-11", "gemm", "f32", 1, 1, 17, 130, 70, 32, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    # f32 64x64
    C("f32-64x64-whole-00", "gemm", "f32", 0, 0, 128, 64, 64, 64, 64, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("f32-64x64-whole-01", "gemm", "f32", 0, 1, 128, 64, 64, 64, 64, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("f32-64x64-whole-10", "gemm", "f32", 1, 0, 128, 64, 64, 64, 64, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("f32-64x64-whole-11", "gemm", "f32", 1, 1, 128, 64, 64, 64, 64, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("f32-64x64-m33-00", "gemm", "f32", 0, 0, 33, 64, 64, 64, 64, PRED, 1, "first M of the 64 x 64 rule", acc=(0, 1)),
    C("f32-64x64-m33-01", "gemm", "f32", 0, 1, 33, 64, 64, 64, 64, PRED, 1, "first M of the 64 x 64 rule", acc=(0, 1)),
    C("f32-64x64-m33-10", "gemm", "f32", 1, 0, 33, 64, 64, 64, 64, PRED, 1, "first M of the 64 x 64 rule", acc=(0, 1)),
    C("f32-64x64-m33-11", "gemm", "f32", 1, 1, 33, 64, 64, 64, 64, PRED, 1, "first M of the 64 x 64 rule", acc=(0, 1)),
    C("f32-64x64-ragM-00", "gemm", "f32", 0, 0, 100, 64, 64, 64, 64, PRED, 1, "ragged M only", acc=(0, 1)),
    C("f32-64x64-ragM-01", "gemm", "f32", 0, 1, 100, 64, 64, 64, 64, PRED, 1, "ragged M only", acc=(0, 1)),
    C("f32-64x64-ragM-10", "gemm", "f32", 1, 0, 100, 64, 64, 64, 64, PRED, 1, "ragged M only", acc=(0, 1)),
    C("f32-64x64-ragM-11", "gemm", "f32", 1, 1, 100, 64, 64, 64, 64, PRED, 1, "ragged M only", acc=(0, 1)),
    C("f32-64x64-ragN-00", "gemm", "f32", 0, 0, 128, 70, 64, 64, 64, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-64x64-ragN-01", "gemm", "f32", 0, 1, 128, 70, 64, 64, 64, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-64x64-ragN-10", "gemm", "f32", 1, 0, 128, 70, 64, 64, 64, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-64x64-ragN-11", "gemm", "f32", 1, 1, 128, 70, 64, 64, 64, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-64x64-ragK-00", "gemm", "f32", 0, 0, 128, 64, 70, 64, 64, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-64x64-ragK-01", "gemm", "f32", 0, 1, 128, 64, 70, 64, 64, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-64x64-ragK-10", "gemm", "f32", 1, 0, 128, 64, 70, 64, 64, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-64x64-ragK-11", "gemm", "f32", 1, 1, 128, 64, 70, 64, 64, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-64x64-ragMNK-00", "gemm", "f32", 0, 0, 100, 70, 70, 64, 64, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-64x64-ragMNK-01", "gemm", "f32", 0, 1, 100, 70, 70, 64, 64, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-64x64-ragMNK-10", "gemm", "f32", 1, 0, 100, 70, 70, 64, 64, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-64x64-ragMNK-11", "gemm", "f32", 1, 1, 100, 70, 70, 64, 64, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-64x64-tall-short-K-00", "gemm", "f32", 0, 0, 1024, 64, 64, 64, 64, FAST, 1, "tall, short K: tile height halved", acc=(0, 1)),
    C("f32-64x64-tall-short-K-01", "gemm", "f32", 0, 1, 1024, 64, 64, 64, 64, FAST, 1, "tall, short K: tile height halved", acc=(0, 1)),
    C("f32-64x64-tall-short-K-10", "gemm", "f32", 1, 0, 1024, 64, 64, 64, 64, FAST, 1, "tall, short K: tile height halved", acc=(0, 1)),
    C("f32-64x64-tall-short-K-11", "gemm", "f32", 1, 1, 1024, 64, 64, 64, 64, FAST, 1, "tall, short K: tile height halved", acc=(0, 1)),
    # f32 128x160
    C("f32-128x160-whole-00", "gemm", "f32", 0, 0, 1024, 160, 512, 128, 160, FAST, 8, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("f32-128x160-whole-01", "gemm", "f32", 0, 1, 1024, 160, 512, 128, 160, FAST, 8, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("f32-128x160-whole-10", "gemm", "f32", 1, 0, 1024, 160, 512, 128, 160, FAST, 8, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("f32-128x160-whole-11", "gemm", "f32", 1, 1, 1024, 160, 512, 128, 160, FAST, 8, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("f32-128x160-ragM-00", "gemm", "f32", 0, 0, 1030, 160, 512, 128, 160, PRED, 8, "ragged M only", acc=(0, 1)),
    C("f32-128x160-ragM-01", "gemm", "f32", 0, 1, 1030, 160, 512, 128, 160, PRED, 8, "ragged M only", acc=(0, 1)),
    C("f32-128x160-ragM-10", "gemm", "f32", 1, 0, 1030, 160, 512, 128, 160, PRED, 8, "ragged M only", acc=(0, 1)),
    C("f32-128x160-ragM-11", "gemm", "f32", 1, 1, 1030, 160, 512, 128, 160, PRED, 8, "ragged M only", acc=(0, 1)),
    C("f32-128x160-ragK-00", "gemm", "f32", 0, 0, 1024, 160, 520, 128, 160, PRED, 7, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-128x160-ragK-01", "gemm", "f32", 0, 1, 1024, 160, 520, 128, 160, PRED, 7, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-128x160-ragK-10", "gemm", "f32", 1, 0, 1024, 160, 520, 128, 160, PRED, 7, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-128x160-ragK-11", "gemm", "f32", 1, 1, 1024, 160, 520, 128, 160, PRED, 7, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-128x160-ragMK-00", "gemm", "f32", 0, 0, 1030, 160, 520, 128, 160, PRED, 7, "ragged M and K", acc=(0, 1)),
    C("f32-128x160-ragMK-01", "gemm", "f32", 0, 1, 1030, 160, 520, 128, 160, PRED, 7, "ragged M and K", acc=(0, 1)),
    C("f32-128x160-ragMK-10", "gemm", "f32", 1, 0, 1030, 160, 520, 128, 160, PRED, 7, "ragged M and K", acc=(0, 1)),
    C("f32-128x160-ragMK-11", "gemm", "f32", 1, 1, 1030, 160, 520, 128, 160, PRED, 7, "ragged M and K", acc=(0, 1)),
    # f32 128x64
    C("f32-128x64-whole-00", "gemm", "f32", 0, 0, 256, 64, 64, 128, 64, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("f32-128x64-whole-01", "gemm", "f32", 0, 1, 256, 64, 64, 128, 64, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("f32-128x64-whole-10", "gemm", "f32", 1, 0, 256, 64, 64, 128, 64, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("f32-128x64-whole-11", "gemm", "f32", 1, 1, 256, 64, 64, 128, 64, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("f32-128x64-ragM-00", "gemm", "f32", 0, 0, 250, 64, 64, 128, 64, PRED, 1, "ragged M only", acc=(0, 1)),
    C("f32-128x64-ragM-01", "gemm", "f32", 0, 1, 250, 64, 64, 128, 64, PRED, 1, "ragged M only", acc=(0, 1)),
    C("f32-128x64-ragM-10", "gemm", "f32", 1, 0, 250, 64, 64, 128, 64, PRED, 1, "ragged M only", acc=(0, 1)),
    C("f32-128x64-ragM-11", "gemm", "f32", 1, 1, 250, 64, 64, 128, 64, PRED, 1, "ragged M only", acc=(0, 1)),
    C("f32-128x64-ragN-00", "gemm", "f32", 0, 0, 256, 50, 64, 128, 64, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-128x64-ragN-01", "gemm", "f32", 0, 1, 256, 50, 64, 128, 64, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-128x64-ragN-10", "gemm", "f32", 1, 0, 256, 50, 64, 128, 64, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-128x64-ragN-11", "gemm", "f32", 1, 1, 256, 50, 64, 128, 64, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-128x64-ragK-00", "gemm", "f32", 0, 0, 256, 64, 70, 128, 64, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-128x64-ragK-01", "gemm", "f32", 0, 1, 256, 64, 70, 128, 64, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-128x64-ragK-10", "gemm", "f32", 1, 0, 256, 64, 70, 128, 64, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-128x64-ragK-11", "gemm", "f32", 1, 1, 256, 64, 70, 128, 64, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-128x64-ragMNK-00", "gemm", "f32", 0, 0, 250, 50, 70, 128, 64, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-128x64-ragMNK-01", "gemm", "f32", 0, 1, 250, 50, 70, 128, 64, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-128x64-ragMNK-10", "gemm", "f32", 1, 0, 250, 50, 70, 128, 64, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-128x64-ragMNK-11", "gemm", "f32", 1, 1, 250, 50, 70, 128, 64, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-128x64-n192-00", "gemm", "f32", 0, 0, 256, 192, 64, 128, 64, FAST, 1, "N a multiple of 64, not of 128", acc=(0, 1)),
    C("f32-128x64-n192-01", "gemm", "f32", 0, 1, 256, 192, 64, 128, 64, FAST, 1, "N a multiple of 64, not of 128", acc=(0, 1)),
    C("f32-128x64-n192-10", "gemm", "f32", 1, 0, 256, 192, 64, 128, 64, FAST, 1, "N a multiple of 64, not of 128", acc=(0, 1)),
    C("f32-128x64-n192-11", "gemm", "f32", 1, 1, 256, 192, 64, 128, 64, FAST, 1, "N a multiple of 64, not of 128", acc=(0, 1)),
    # f32 64x128
    C("f32-64x128-whole-00", "gemm", "f32", 0, 0, 192, 128, 64, 64, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("f32-64x128-whole-01", "gemm", "f32", 0, 1, 192, 128, 64, 64, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("f32-64x128-whole-10", "gemm", "f32", 1, 0, 192, 128, 64, 64, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("f32-64x128-whole-11", "gemm", "f32", 1, 1, 192, 128, 64, 64, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("f32-64x128-ragN-00", "gemm", "f32", 0, 0, 192, 130, 64, 64, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-64x128-ragN-01", "gemm", "f32", 0, 1, 192, 130, 64, 64, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-64x128-ragN-10", "gemm", "f32", 1, 0, 192, 130, 64, 64, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-64x128-ragN-11", "gemm", "f32", 1, 1, 192, 130, 64, 64, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-64x128-ragK-00", "gemm", "f32", 0, 0, 192, 128, 70, 64, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-64x128-ragK-01", "gemm", "f32", 0, 1, 192, 128, 70, 64, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-64x128-ragK-10", "gemm", "f32", 1, 0, 192, 128, 70, 64, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-64x128-ragK-11", "gemm", "f32", 1, 1, 192, 128, 70, 64, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-64x128-ragNK-00", "gemm", "f32", 0, 0, 192, 130, 70, 64, 128, PRED, 1, "ragged N and K", acc=(0, 1)),
    C("f32-64x128-ragNK-01", "gemm", "f32", 0, 1, 192, 130, 70, 64, 128, PRED, 1, "ragged N and K", acc=(0, 1)),
    C("f32-64x128-ragNK-10", "gemm", "f32", 1, 0, 192, 130, 70, 64, 128, PRED, 1, "ragged N and K", acc=(0, 1)),
    C("f32-64x128-ragNK-11", "gemm", "f32", 1, 1, 192, 130, 70, 64, 128, PRED, 1, "ragged N and K", acc=(0, 1)),
    C("f32-64x128-tall-short-K-00", "gemm", "f32", 0, 0, 1024, 128, 64, 64, 128, FAST, 1, "tall, short K: tile height halved", acc=(0, 1)),
    C("f32-64x128-tall-short-K-01", "gemm", "f32", 0, 1, 1024, 128, 64, 64, 128, FAST, 1, "tall, short K: tile height halved", acc=(0, 1)),
    C("f32-64x128-tall-short-K-10", "gemm", "f32", 1, 0, 1024, 128, 64, 64, 128, FAST, 1, "tall, short K: tile height halved", acc=(0, 1)),
    C("f32-64x128-tall-short-K-11", "gemm", "f32", 1, 1, 1024, 128, 64, 64, 128, FAST, 1, "tall, short K: tile height halved", acc=(0, 1)),
    C("f32-64x128-tall-ragM-00", "gemm", "f32", 0, 0, 1030, 128, 64, 64, 128, PRED, 1, "halved tile, ragged M", acc=(0, 1)),
    C("f32-64x128-tall-ragM-01", "gemm", "f32", 0, 1, 1030, 128, 64, 64, 128, PRED, 1, "halved tile, ragged M", acc=(0, 1)),
    C("f32-64x128-tall-ragM-10", "gemm", "f32", 1, 0, 1030, 128, 64, 64, 128, PRED, 1, "halved tile, ragged M", acc=(0, 1)),
    C("f32-64x128-tall-ragM-11", "gemm", "f32", 1, 1, 1030, 128, 64, 64, 128, PRED, 1, "halved tile, ragged M", acc=(0, 1)),
    C("f32-64x128-tall-ragMNK-00", "gemm", "f32", 0, 0, 1030, 130, 70, 64, 128, PRED, 1, "halved tile, ragged M, N, K", acc=(0, 1)),
    C("f32-64x128-tall-ragMNK-01", "gemm", "f32", 0, 1, 1030, 130, 70, 64, 128, PRED, 1, "halved tile, ragged M, N, K", acc=(0, 1)),
    C("f32-64x128-tall-ragMNK-10", "gemm", "f32", 1, 0, 1030, 130, 70, 64, 128, PRED, 1, "halved tile, ragged M, N, K", acc=(0, 1)),
    C("f32-64x128-tall-ragMNK-11", "gemm", "f32", 1, 1, 1030, 130, 70, 64, 128, PRED, 1, "halved tile, ragged M, N, K", acc=(0, 1)),
    # f32 128x128
    C("f32-128x128-whole-00", "gemm", "f32", 0, 0, 256, 128, 64, 128, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("f32-128x128-whole-01", "gemm", "f32", 0, 1, 256, 128, 64, 128, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("f32-128x128-whole-10", "gemm", "f32", 1, 0, 256, 128, 64, 128, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("f32-128x128-whole-11", "gemm", "f32", 1, 1, 256, 128, 64, 128, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("f32-128x128-ragM-00", "gemm", "f32", 0, 0, 250, 128, 64, 128, 128, PRED, 1, "ragged M only", acc=(0, 1)),
    C("f32-128x128-ragM-01", "gemm", "f32", 0, 1, 250, 128, 64, 128, 128, PRED, 1, "ragged M only", acc=(0, 1)),
    C("f32-128x128-ragM-10", "gemm", "f32", 1, 0, 250, 128, 64, 128, 128, PRED, 1, "ragged M only", acc=(0, 1)),
    C("f32-128x128-ragM-11", "gemm", "f32", 1, 1, 250, 128, 64, 128, 128, PRED, 1, "ragged M only", acc=(0, 1)),
    C("f32-128x128-ragN-00", "gemm", "f32", 0, 0, 256, 130, 64, 128, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-128x128-ragN-01", "gemm", "f32", 0, 1, 256, 130, 64, 128, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-128x128-ragN-10", "gemm", "f32", 1, 0, 256, 130, 64, 128, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-128x128-ragN-11", "gemm", "f32", 1, 1, 256, 130, 64, 128, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("f32-128x128-ragK-00", "gemm", "f32", 0, 0, 256, 128, 70, 128, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-128x128-ragK-01", "gemm", "f32", 0, 1, 256, 128, 70, 128, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-128x128-ragK-10", "gemm", "f32", 1, 0, 256, 128, 70, 128, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-128x128-ragK-11", "gemm", "f32", 1, 1, 256, 128, 70, 128, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("f32-128x128-ragMNK-00", "gemm", "f32", 0, 0, 250, 130, 70, 128, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-128x128-ragMNK-01", "gemm", "f32", 0, 1, 250, 130, 70, 128, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-128x128-ragMNK-10", "gemm", "f32", 1, 0, 250, 130, 70, 128, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("f32-128x128-ragMNK-11", "gemm", "f32", 1, 1, 250, 130, 70, 128, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    # bf16 32x128
    C("bf16-32x128-whole-00", "gemm", "bf16", 0, 0, 32, 128, 64, 32, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("bf16-32x128-whole-01", "gemm", "bf16", 0, 1, 32, 128, 64, 32, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("bf16-32x128-whole-10", "gemm", "bf16", 1, 0, 32, 128, 64, 32, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("bf16-32x128-whole-11", "gemm", "bf16", 1, 1, 32, 128, 64, 32, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("bf16-32x128-m1-00", "gemm", "bf16", 0, 0, 1, 128, 64, 32, 128, PRED, 1, "one row", acc=(0, 1)),
    C("bf16-32x128-m1-01", "gemm", "bf16", 0, 1, 1, 128, 64, 32, 128, PRED, 1, "one row", acc=(0, 1)),
    C("bf16-32x128-m1-10", "gemm", "bf16", 1, 0, 1, 128, 64, 32, 128, PRED, 1, "one row", acc=(0, 1)),
    C("bf16-32x128-m1-11", "gemm", "bf16", 1, 1, 1, 128, 64, 32, 128, PRED, 1, "one row", acc=(0, 1)),
    C("bf16-32x128-ragN-00", "gemm", "bf16", 0, 0, 32, 130, 64, 32, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-32x128-ragN-01", "gemm", "bf16", 0, 1, 32, 130, 64, 32, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-32x128-ragN-10", "gemm", "bf16", 1, 0, 32, 130, 64, 32, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-32x128-ragN-11", "gemm", "bf16", 1, 1, 32, 130, 64, 32, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-32x128-ragK-00", "gemm", "bf16", 0, 0, 32, 128, 70, 32, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-32x128-ragK-01", "gemm", "bf16", 0, 1, 32, 128, 70, 32, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-32x128-ragK-10", "gemm", "bf16", 1, 0, 32, 128, 70, 32, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-32x128-ragK-11", "gemm", "bf16", 1, 1, 32, 128, 70, 32, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-32x128-ragMNK-00", "gemm", "bf16", 0, 0, 17, 130, 70, 32, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("bf16-32x128-ragMNK-01", "gemm", "bf16", 0, 1, 17, 130, 70, 32, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("bf16-32x128-ragMNK-10", "gemm", "bf16", 1, 0, 17, 130, 70, 32, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("bf16-32x128-ragMNK-11", "gemm", "bf16", 1, 1, 17, 130, 70, 32, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    # bf16 128x160
    C("bf16-128x160-whole-00", "gemm", "bf16", 0, 0, 1024, 160, 64, 128, 160, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("bf16-128x160-whole-01", "gemm", "bf16", 0, 1, 1024, 160, 64, 128, 160, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("bf16-128x160-whole-10", "gemm", "bf16", 1, 0, 1024, 160, 64, 128, 160, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("bf16-128x160-whole-11", "gemm", "bf16", 1, 1, 1024, 160, 64, 128, 160, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("bf16-128x160-ragM-00", "gemm", "bf16", 0, 0, 1030, 160, 64, 128, 160, PRED, 1, "ragged M only", acc=(0, 1)),
    C("bf16-128x160-ragM-01", "gemm", "bf16", 0, 1, 1030, 160, 64, 128, 160, PRED, 1, "ragged M only", acc=(0, 1)),
    C("bf16-128x160-ragM-10", "gemm", "bf16", 1, 0, 1030, 160, 64, 128, 160, PRED, 1, "ragged M only", acc=(0, 1)),
    C("bf16-128x160-ragM-11", "gemm", "bf16", 1, 1, 1030, 160, 64, 128, 160, PRED, 1, "ragged M only", acc=(0, 1)),
    C("bf16-128x160-ragK-00", "gemm", "bf16", 0, 0, 1024, 160, 70, 128, 160, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-128x160-ragK-01", "gemm", "bf16", 0, 1, 1024, 160, 70, 128, 160, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-128x160-ragK-10", "gemm", "bf16", 1, 0, 1024, 160, 70, 128, 160, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-128x160-ragK-11", "gemm", "bf16", 1, 1, 1024, 160, 70, 128, 160, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-128x160-ragMK-00", "gemm", "bf16", 0, 0, 1030, 160, 70, 128, 160, PRED, 1, "ragged M and K", acc=(0, 1)),
    C("bf16-128x160-ragMK-01", "gemm", "bf16", 0, 1, 1030, 160, 70, 128, 160, PRED, 1, "ragged M and K", acc=(0, 1)),
    C("bf16-128x160-ragMK-10", "gemm", "bf16", 1, 0, 1030, 160, 70, 128, 160, PRED, 1, "ragged M and K", acc=(0, 1)),
    C("bf16-128x160-ragMK-11", "gemm", "bf16", 1, 1, 1030, 160, 70, 128, 160, PRED, 1, "ragged M and K", acc=(0, 1)),
    # bf16 160x128
    C("bf16-160x128-whole-00", "gemm", "bf16", 0, 0, 160, 128, 65536, 160, 128, FAST, 256, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("bf16-160x128-whole-01", "gemm", "bf16", 0, 1, 160, 128, 65536, 160, 128, FAST, 256, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("bf16-160x128-whole-10", "gemm", "bf16", 1, 0, 160, 128, 65536, 160, 128, FAST, 256, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("bf16-160x128-whole-11", "gemm", "bf16", 1, 1, 160, 128, 65536, 160, 128, FAST, 256, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("bf16-160x128-ragK-00", "gemm", "bf16", 0, 0, 160, 128, 65544, 160, 128, PRED, 228, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-160x128-ragK-01", "gemm", "bf16", 0, 1, 160, 128, 65544, 160, 128, PRED, 228, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-160x128-ragK-10", "gemm", "bf16", 1, 0, 160, 128, 65544, 160, 128, PRED, 228, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-160x128-ragK-11", "gemm", "bf16", 1, 1, 160, 128, 65544, 160, 128, PRED, 228, "K not a multiple of the slab", acc=(0, 1)),
    # bf16 128x64
    C("bf16-128x64-whole-00", "gemm", "bf16", 0, 0, 256, 64, 64, 128, 64, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("bf16-128x64-whole-01", "gemm", "bf16", 0, 1, 256, 64, 64, 128, 64, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("bf16-128x64-whole-10", "gemm", "bf16", 1, 0, 256, 64, 64, 128, 64, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("bf16-128x64-whole-11", "gemm", "bf16", 1, 1, 256, 64, 64, 128, 64, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("bf16-128x64-ragM-00", "gemm", "bf16", 0, 0, 250, 64, 64, 128, 64, PRED, 1, "ragged M only", acc=(0, 1)),
    C("bf16-128x64-ragM-01", "gemm", "bf16", 0, 1, 250, 64, 64, 128, 64, PRED, 1, "ragged M only", acc=(0, 1)),
    C("bf16-128x64-ragM-10", "gemm", "bf16", 1, 0, 250, 64, 64, 128, 64, PRED, 1, "ragged M only", acc=(0, 1)),
    C("bf16-128x64-ragM-11", "gemm", "bf16", 1, 1, 250, 64, 64, 128, 64, PRED, 1, "ragged M only", acc=(0, 1)),
    C("bf16-128x64-ragN-00", "gemm", "bf16", 0, 0, 256, 50, 64, 128, 64, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-128x64-ragN-01", "gemm", "bf16", 0, 1, 256, 50, 64, 128, 64, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-128x64-ragN-10", "gemm", "bf16", 1, 0, 256, 50, 64, 128, 64, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-128x64-ragN-11", "gemm", "bf16", 1, 1, 256, 50, 64, 128, 64, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-128x64-ragK-00", "gemm", "bf16", 0, 0, 256, 64, 70, 128, 64, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-128x64-ragK-01", "gemm", "bf16", 0, 1, 256, 64, 70, 128, 64, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-128x64-ragK-10", "gemm", "bf16", 1, 0, 256, 64, 70, 128, 64, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-128x64-ragK-11", "gemm", "bf16", 1, 1, 256, 64, 70, 128, 64, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-128x64-ragMNK-00", "gemm", "bf16", 0, 0, 250, 50, 70, 128, 64, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("bf16-128x64-ragMNK-01", "gemm", "bf16", 0, 1, 250, 50, 70, 128, 64, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("bf16-128x64-ragMNK-10", "gemm", "bf16", 1, 0, 250, 50, 70, 128, 64, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("bf16-128x64-ragMNK-11", "gemm", "bf16", 1, 1, 250, 50, 70, 128, 64, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    # bf16 64x128
    C("bf16-64x128-whole-00", "gemm", "bf16", 0, 0, 192, 128, 64, 64, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("bf16-64x128-whole-01", "gemm", "bf16", 0, 1, 192, 128, 64, 64, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("bf16-64x128-whole-10", "gemm", "bf16", 1, 0, 192, 128, 64, 64, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("bf16-64x128-whole-11", "gemm", "bf16", 1, 1, 192, 128, 64, 64, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("bf16-64x128-ragN-00", "gemm", "bf16", 0, 0, 192, 130, 64, 64, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-64x128-ragN-01", "gemm", "bf16", 0, 1, 192, 130, 64, 64, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-64x128-ragN-10", "gemm", "bf16", 1, 0, 192, 130, 64, 64, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-64x128-ragN-11", "gemm", "bf16", 1, 1, 192, 130, 64, 64, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-64x128-ragK-00", "gemm", "bf16", 0, 0, 192, 128, 70, 64, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-64x128-ragK-01", "gemm", "bf16", 0, 1, 192, 128, 70, 64, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-64x128-ragK-10", "gemm", "bf16", 1, 0, 192, 128, 70, 64, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-64x128-ragK-11", "gemm", "bf16", 1, 1, 192, 128, 70, 64, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-64x128-ragNK-00", "gemm", "bf16", 0, 0, 192, 130, 70, 64, 128, PRED, 1, "ragged N and K", acc=(0, 1)),
    C("bf16-64x128-ragNK-01", "gemm", "bf16", 0, 1, 192, 130, 70, 64, 128, PRED, 1, "ragged N and K", acc=(0, 1)),
    C("bf16-64x128-ragNK-10", "gemm", "bf16", 1, 0, 192, 130, 70, 64, 128, PRED, 1, "ragged N and K", acc=(0, 1)),
    C("bf16-64x128-ragNK-11", "gemm", "bf16", 1, 1, 192, 130, 70, 64, 128, PRED, 1, "ragged N and K", acc=(0, 1)),
    # bf16 128x128
    C("bf16-128x128-whole-00", "gemm", "bf16", 0, 0, 256, 128, 64, 128, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("bf16-128x128-whole-01", "gemm", "bf16", 0, 1, 256, 128, 64, 128, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=0),
    C("bf16-128x128-whole-10", "gemm", "bf16", 1, 0, 256, 128, 64, 128, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("bf16-128x128-whole-11", "gemm", "bf16", 1, 1, 256, 128, 64, 128, 128, FAST, 1, "whole tiles and slabs, aligned", acc=(0, 1), lda_extra=8, ldb_extra=4, ldc_extra=4),
    C("bf16-128x128-ragM-00", "gemm", "bf16", 0, 0, 250, 128, 64, 128, 128, PRED, 1, "ragged M only", acc=(0, 1)),
    C("bf16-128x128-ragM-01", "gemm", "bf16", 0, 1, 250, 128, 64, 128, 128, PRED, 1, "ragged M only", acc=(0, 1)),
    C("bf16-128x128-ragM-10", "gemm", "bf16", 1, 0, 250, 128, 64, 128, 128, PRED, 1, "ragged M only", acc=(0, 1)),
    C("bf16-128x128-ragM-11", "gemm", "bf16", 1, 1, 250, 128, 64, 128, 128, PRED, 1, "ragged M only", acc=(0, 1)),
    C("bf16-128x128-ragN-00", "gemm", "bf16", 0, 0, 256, 130, 64, 128, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-128x128-ragN-01", "gemm", "bf16", 0, 1, 256, 130, 64, 128, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-128x128-ragN-10", "gemm", "bf16", 1, 0, 256, 130, 64, 128, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-128x128-ragN-11", "gemm", "bf16", 1, 1, 256, 130, 64, 128, 128, PRED, 1, "ragged N only", acc=(0, 1)),
    C("bf16-128x128-ragK-00", "gemm", "bf16", 0, 0, 256, 128, 70, 128, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-128x128-ragK-01", "gemm", "bf16", 0, 1, 256, 128, 70, 128, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-128x128-ragK-10", "gemm", "bf16", 1, 0, 256, 128, 70, 128, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-128x128-ragK-11", "gemm", "bf16", 1, 1, 256, 128, 70, 128, 128, PRED, 1, "K not a multiple of the slab", acc=(0, 1)),
    C("bf16-128x128-ragMNK-00", "gemm", "bf16", 0, 0, 250, 130, 70, 128, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("bf16-128x128-ragMNK-01", "gemm", "bf16", 0, 1, 250, 130, 70, 128, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("bf16-128x128-ragMNK-10", "gemm", "bf16", 1, 0, 250, 130, 70, 128, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    C("bf16-128x128-ragMNK-11", "gemm", "bf16", 1, 1, 250, 130, 70, 128, 128, PRED, 1, "ragged M, N and K", acc=(0, 1)),
    # alignment: whole shapes, so the operand's alignment is the only reason to leave the predicate-free kernel
    C("f32-align-A-ld+1-00", "gemm", "f32", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "A ld % 4 != 0, aligned base", lda_extra=1),
    C("f32-align-A-ld+2-00", "gemm", "f32", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "A ld % 4 != 0, aligned base", lda_extra=2),
    C("f32-align-A-off1-00", "gemm", "f32", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "A base off by 1 floats, ld % 4 == 0", a_off=1),
    C("f32-align-A-off2-00", "gemm", "f32", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "A base off by 2 floats, ld % 4 == 0", a_off=2),
    C("f32-align-A-off3-00", "gemm", "f32", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "A base off by 3 floats, ld % 4 == 0", a_off=3),
    C("f32-align-B-ld+1-00", "gemm", "f32", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "B ld % 4 != 0, aligned base", ldb_extra=1),
    C("f32-align-B-ld+2-00", "gemm", "f32", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "B ld % 4 != 0, aligned base", ldb_extra=2),
    C("f32-align-B-off1-00", "gemm", "f32", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "B base off by 1 floats, ld % 4 == 0", b_off=1),
    C("f32-align-B-off2-00", "gemm", "f32", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "B base off by 2 floats, ld % 4 == 0", b_off=2),
    C("f32-align-B-off3-00", "gemm", "f32", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "B base off by 3 floats, ld % 4 == 0", b_off=3),
    C("f32-align-A-ld+1-11", "gemm", "f32", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "A ld % 4 != 0, aligned base", lda_extra=1),
    C("f32-align-A-ld+2-11", "gemm", "f32", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "A ld % 4 != 0, aligned base", lda_extra=2),
    C("f32-align-A-off1-11", "gemm", "f32", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "A base off by 1 floats, ld % 4 == 0", a_off=1),
    C("f32-align-A-off2-11", "gemm", "f32", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "A base off by 2 floats, ld % 4 == 0", a_off=2),
    C("f32-align-A-off3-11", "gemm", "f32", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "A base off by 3 floats, ld % 4 == 0", a_off=3),
    C("f32-align-B-ld+1-11", "gemm", "f32", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "B ld % 4 != 0, aligned base", ldb_extra=1),
    C("f32-align-B-ld+2-11", "gemm", "f32", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "B ld % 4 != 0, aligned base", ldb_extra=2),
    C("f32-align-B-off1-11", "gemm", "f32", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "B base off by 1 floats, ld % 4 == 0", b_off=1),
    C("f32-align-B-off2-11", "gemm", "f32", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "B base off by 2 floats, ld % 4 == 0", b_off=2),
    C("f32-align-B-off3-11", "gemm", "f32", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "B base off by 3 floats, ld % 4 == 0", b_off=3),
    C("bf16-align-A-ld+1-00", "gemm", "bf16", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "A ld % 4 != 0, aligned base", lda_extra=1),
    C("bf16-align-A-ld+2-00", "gemm", "bf16", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "A ld % 4 != 0, aligned base", lda_extra=2),
    C("bf16-align-A-off1-00", "gemm", "bf16", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "A base off by 1 floats, ld % 4 == 0", a_off=1),
    C("bf16-align-A-off2-00", "gemm", "bf16", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "A base off by 2 floats, ld % 4 == 0", a_off=2),
    C("bf16-align-A-off3-00", "gemm", "bf16", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "A base off by 3 floats, ld % 4 == 0", a_off=3),
    C("bf16-align-B-ld+1-00", "gemm", "bf16", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "B ld % 4 != 0, aligned base", ldb_extra=1),
    C("bf16-align-B-ld+2-00", "gemm", "bf16", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "B ld % 4 != 0, aligned base", ldb_extra=2),
    C("bf16-align-B-off1-00", "gemm", "bf16", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "B base off by 1 floats, ld % 4 == 0", b_off=1),
    C("bf16-align-B-off2-00", "gemm", "bf16", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "B base off by 2 floats, ld % 4 == 0", b_off=2),
    C("bf16-align-B-off3-00", "gemm", "bf16", 0, 0, 256, 128, 64, 128, 128, PRED, 1, "B base off by 3 floats, ld % 4 == 0", b_off=3),
    C("bf16-align-A-ld+1-11", "gemm", "bf16", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "A ld % 4 != 0, aligned base", lda_extra=1),
    C("bf16-align-A-ld+2-11", "gemm", "bf16", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "A ld % 4 != 0, aligned base", lda_extra=2),
    C("bf16-align-A-off1-11", "gemm", "bf16", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "A base off by 1 floats, ld % 4 == 0", a_off=1),
    C("bf16-align-A-off2-11", "gemm", "bf16", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "A base off by 2 floats, ld % 4 == 0", a_off=2),
    C("bf16-align-A-off3-11", "gemm", "bf16", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "A base off by 3 floats, ld % 4 == 0", a_off=3),
    C("bf16-align-B-ld+1-11", "gemm", "bf16", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "B ld % 4 != 0, aligned base", ldb_extra=1),
    C("bf16-align-B-ld+2-11", "gemm", "bf16", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "B ld % 4 != 0, aligned base", ldb_extra=2),
    C("bf16-align-B-off1-11", "gemm", "bf16", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "B base off by 1 floats, ld % 4 == 0", b_off=1),
    C("bf16-align-B-off2-11", "gemm", "bf16", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "B base off by 2 floats, ld % 4 == 0", b_off=2),
    C("bf16-align-B-off3-11", "gemm", "bf16", 1, 1, 256, 128, 64, 128, 128, PRED, 1, "B base off by 3 floats, ld % 4 == 0", b_off=3),
    # K cuts (slices from the _splits query), every epilogue: store + clear pass, add, known-zero output
    C("f32-cut-1-00", "gemm", "f32", 0, 0, 256, 128, 64, 128, 128, FAST, 1, "one slice", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-1-01", "gemm", "f32", 0, 1, 256, 128, 64, 128, 128, FAST, 1, "one slice", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-1-10", "gemm", "f32", 1, 0, 256, 128, 64, 128, 128, FAST, 1, "one slice", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-1-11", "gemm", "f32", 1, 1, 256, 128, 64, 128, 128, FAST, 1, "one slice", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-2-00", "gemm", "f32", 0, 0, 256, 128, 128, 128, 128, FAST, 2, "two slices", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-2-01", "gemm", "f32", 0, 1, 256, 128, 128, 128, 128, FAST, 2, "two slices", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-2-10", "gemm", "f32", 1, 0, 256, 128, 128, 128, 128, FAST, 2, "two slices", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-2-11", "gemm", "f32", 1, 1, 256, 128, 128, 128, 128, FAST, 2, "two slices", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-3-00", "gemm", "f32", 0, 0, 256, 128, 192, 128, 128, FAST, 3, "three slices", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-3-01", "gemm", "f32", 0, 1, 256, 128, 192, 128, 128, FAST, 3, "three slices", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-3-10", "gemm", "f32", 1, 0, 256, 128, 192, 128, 128, FAST, 3, "three slices", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-3-11", "gemm", "f32", 1, 1, 256, 128, 192, 128, 128, FAST, 3, "three slices", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-8-00", "gemm", "f32", 0, 0, 256, 128, 512, 128, 128, FAST, 8, "exactly 8: one slice per XCD", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-8-01", "gemm", "f32", 0, 1, 256, 128, 512, 128, 128, FAST, 8, "exactly 8: one slice per XCD", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-8-10", "gemm", "f32", 1, 0, 256, 128, 512, 128, 128, FAST, 8, "exactly 8: one slice per XCD", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-8-11", "gemm", "f32", 1, 1, 256, 128, 512, 128, 128, FAST, 8, "exactly 8: one slice per XCD", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-16-00", "gemm", "f32", 0, 0, 256, 128, 1024, 128, 128, FAST, 16, "16: whole slices per XCD", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-16-01", "gemm", "f32", 0, 1, 256, 128, 1024, 128, 128, FAST, 16, "16: whole slices per XCD", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-16-10", "gemm", "f32", 1, 0, 256, 128, 1024, 128, 128, FAST, 16, "16: whole slices per XCD", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-16-11", "gemm", "f32", 1, 1, 256, 128, 1024, 128, 128, FAST, 16, "16: whole slices per XCD", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-20to16-00", "gemm", "f32", 0, 0, 256, 128, 1280, 128, 128, FAST, 16, "K / 64 = 20 rounded down to 16", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-20to16-01", "gemm", "f32", 0, 1, 256, 128, 1280, 128, 128, FAST, 16, "K / 64 = 20 rounded down to 16", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-20to16-10", "gemm", "f32", 1, 0, 256, 128, 1280, 128, 128, FAST, 16, "K / 64 = 20 rounded down to 16", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-20to16-11", "gemm", "f32", 1, 1, 256, 128, 1280, 128, 128, FAST, 16, "K / 64 = 20 rounded down to 16", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-lastshort-00", "gemm", "f32", 0, 0, 256, 128, 200, 128, 128, PRED, 3, "3 slices of 80, 80, 40", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-lastshort-01", "gemm", "f32", 0, 1, 256, 128, 200, 128, 128, PRED, 3, "3 slices of 80, 80, 40", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-lastshort-10", "gemm", "f32", 1, 0, 256, 128, 200, 128, 128, PRED, 3, "3 slices of 80, 80, 40", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-lastshort-11", "gemm", "f32", 1, 1, 256, 128, 200, 128, 128, PRED, 3, "3 slices of 80, 80, 40", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-fewer8to7-00", "gemm", "f32", 0, 0, 256, 128, 520, 128, 128, PRED, 7, "plan asks 8, slices of 80 give 7", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-fewer8to7-01", "gemm", "f32", 0, 1, 256, 128, 520, 128, 128, PRED, 7, "plan asks 8, slices of 80 give 7", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-fewer8to7-10", "gemm", "f32", 1, 0, 256, 128, 520, 128, 128, PRED, 7, "plan asks 8, slices of 80 give 7", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-fewer8to7-11", "gemm", "f32", 1, 1, 256, 128, 520, 128, 128, PRED, 7, "plan asks 8, slices of 80 give 7", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-fewer16to14-00", "gemm", "f32", 0, 0, 256, 128, 1088, 128, 128, PRED, 14, "plan asks 16, slices of 80 give 14", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-fewer16to14-01", "gemm", "f32", 0, 1, 256, 128, 1088, 128, 128, PRED, 14, "plan asks 16, slices of 80 give 14", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-fewer16to14-10", "gemm", "f32", 1, 0, 256, 128, 1088, 128, 128, PRED, 14, "plan asks 16, slices of 80 give 14", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-fewer16to14-11", "gemm", "f32", 1, 1, 256, 128, 1088, 128, 128, PRED, 14, "plan asks 16, slices of 80 give 14", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-rag-8-00", "gemm", "f32", 0, 0, 250, 130, 512, 128, 128, PRED, 8, "8 slices, ragged tiles", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-rag-8-01", "gemm", "f32", 0, 1, 250, 130, 512, 128, 128, PRED, 8, "8 slices, ragged tiles", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-rag-8-10", "gemm", "f32", 1, 0, 250, 130, 512, 128, 128, PRED, 8, "8 slices, ragged tiles", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-rag-8-11", "gemm", "f32", 1, 1, 250, 130, 512, 128, 128, PRED, 8, "8 slices, ragged tiles", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-k131071-00", "gemm", "f32", 0, 0, 64, 64, 131071, 64, 64, PRED, 256, "largest K with a = 8, ragged", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-k131071-10", "gemm", "f32", 1, 0, 64, 64, 131071, 64, 64, PRED, 256, "largest K with a = 8, ragged", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-k262144-00", "gemm", "f32", 0, 0, 32, 128, 262144, 32, 128, FAST, 256, "a = 4", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-k262144-10", "gemm", "f32", 1, 0, 32, 128, 262144, 32, 128, FAST, 256, "a = 4", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-64x64-10tiles-00", "gemm", "f32", 0, 0, 128, 320, 4096, 64, 64, FAST, 64, "64 x 64, ten tiles", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-64x64-10tiles-01", "gemm", "f32", 0, 1, 128, 320, 4096, 64, 64, FAST, 64, "64 x 64, ten tiles", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-64x64-10tiles-10", "gemm", "f32", 1, 0, 128, 320, 4096, 64, 64, FAST, 64, "64 x 64, ten tiles", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-64x64-10tiles-11", "gemm", "f32", 1, 1, 128, 320, 4096, 64, 64, FAST, 64, "64 x 64, ten tiles", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-160-32tiles-00", "gemm", "f32", 0, 0, 2048, 320, 512, 128, 160, FAST, 8, "128 x 160, 32 tiles", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-160-32tiles-01", "gemm", "f32", 0, 1, 2048, 320, 512, 128, 160, FAST, 8, "128 x 160, 32 tiles", acc=(0, 1, 2), ldc_extra=4),
    C("f32-cut-160-32tiles-10", "gemm", "f32", 1, 0, 2048, 320, 512, 128, 160, FAST, 8, "128 x 160, 32 tiles", acc=(0, 1, 2), ldc_extra=0),
    C("f32-cut-160-32tiles-11", "gemm", "f32", 1, 1, 2048, 320, 512, 128, 160, FAST, 8, "128 x 160, 32 tiles", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-1-00", "gemm", "bf16", 0, 0, 256, 128, 64, 128, 128, FAST, 1, "one slice", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-1-01", "gemm", "bf16", 0, 1, 256, 128, 64, 128, 128, FAST, 1, "one slice", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-1-10", "gemm", "bf16", 1, 0, 256, 128, 64, 128, 128, FAST, 1, "one slice", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-1-11", "gemm", "bf16", 1, 1, 256, 128, 64, 128, 128, FAST, 1, "one slice", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-2-00", "gemm", "bf16", 0, 0, 256, 128, 256, 128, 128, FAST, 2, "two slices", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-2-01", "gemm", "bf16", 0, 1, 256, 128, 256, 128, 128, FAST, 2, "two slices", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-2-10", "gemm", "bf16", 1, 0, 256, 128, 256, 128, 128, FAST, 2, "two slices", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-2-11", "gemm", "bf16", 1, 1, 256, 128, 256, 128, 128, FAST, 2, "two slices", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-3-00", "gemm", "bf16", 0, 0, 256, 128, 384, 128, 128, FAST, 3, "three slices", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-3-01", "gemm", "bf16", 0, 1, 256, 128, 384, 128, 128, FAST, 3, "three slices", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-3-10", "gemm", "bf16", 1, 0, 256, 128, 384, 128, 128, FAST, 3, "three slices", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-3-11", "gemm", "bf16", 1, 1, 256, 128, 384, 128, 128, FAST, 3, "three slices", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-8-00", "gemm", "bf16", 0, 0, 256, 128, 1024, 128, 128, FAST, 8, "exactly 8: one slice per XCD", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-8-01", "gemm", "bf16", 0, 1, 256, 128, 1024, 128, 128, FAST, 8, "exactly 8: one slice per XCD", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-8-10", "gemm", "bf16", 1, 0, 256, 128, 1024, 128, 128, FAST, 8, "exactly 8: one slice per XCD", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-8-11", "gemm", "bf16", 1, 1, 256, 128, 1024, 128, 128, FAST, 8, "exactly 8: one slice per XCD", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-16-00", "gemm", "bf16", 0, 0, 256, 128, 2048, 128, 128, FAST, 16, "16: whole slices per XCD", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-16-01", "gemm", "bf16", 0, 1, 256, 128, 2048, 128, 128, FAST, 16, "16: whole slices per XCD", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-16-10", "gemm", "bf16", 1, 0, 256, 128, 2048, 128, 128, FAST, 16, "16: whole slices per XCD", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-16-11", "gemm", "bf16", 1, 1, 256, 128, 2048, 128, 128, FAST, 16, "16: whole slices per XCD", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-20to16-00", "gemm", "bf16", 0, 0, 256, 128, 2560, 128, 128, FAST, 16, "K / 128 = 20 rounded down to 16", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-20to16-01", "gemm", "bf16", 0, 1, 256, 128, 2560, 128, 128, FAST, 16, "K / 128 = 20 rounded down to 16", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-20to16-10", "gemm", "bf16", 1, 0, 256, 128, 2560, 128, 128, FAST, 16, "K / 128 = 20 rounded down to 16", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-20to16-11", "gemm", "bf16", 1, 1, 256, 128, 2560, 128, 128, FAST, 16, "K / 128 = 20 rounded down to 16", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-lastshort-00", "gemm", "bf16", 0, 0, 256, 128, 400, 128, 128, PRED, 3, "3 slices of 160, 160, 80", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-lastshort-01", "gemm", "bf16", 0, 1, 256, 128, 400, 128, 128, PRED, 3, "3 slices of 160, 160, 80", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-lastshort-10", "gemm", "bf16", 1, 0, 256, 128, 400, 128, 128, PRED, 3, "3 slices of 160, 160, 80", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-lastshort-11", "gemm", "bf16", 1, 1, 256, 128, 400, 128, 128, PRED, 3, "3 slices of 160, 160, 80", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-lastshort-whole-00", "gemm", "bf16", 0, 0, 256, 128, 416, 128, 128, FAST, 3, "160, 160, 96: short last slice in the predicate-free kernel", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-lastshort-whole-01", "gemm", "bf16", 0, 1, 256, 128, 416, 128, 128, FAST, 3, "160, 160, 96: short last slice in the predicate-free kernel", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-lastshort-whole-10", "gemm", "bf16", 1, 0, 256, 128, 416, 128, 128, FAST, 3, "160, 160, 96: short last slice in the predicate-free kernel", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-lastshort-whole-11", "gemm", "bf16", 1, 1, 256, 128, 416, 128, 128, FAST, 3, "160, 160, 96: short last slice in the predicate-free kernel", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-fewer8to7-00", "gemm", "bf16", 0, 0, 256, 128, 1056, 128, 128, FAST, 7, "plan asks 8, slices of 160 give 7", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-fewer8to7-01", "gemm", "bf16", 0, 1, 256, 128, 1056, 128, 128, FAST, 7, "plan asks 8, slices of 160 give 7", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-fewer8to7-10", "gemm", "bf16", 1, 0, 256, 128, 1056, 128, 128, FAST, 7, "plan asks 8, slices of 160 give 7", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-fewer8to7-11", "gemm", "bf16", 1, 1, 256, 128, 1056, 128, 128, FAST, 7, "plan asks 8, slices of 160 give 7", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-rag-8-00", "gemm", "bf16", 0, 0, 250, 130, 1024, 128, 128, PRED, 8, "8 slices, ragged tiles", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-rag-8-01", "gemm", "bf16", 0, 1, 250, 130, 1024, 128, 128, PRED, 8, "8 slices, ragged tiles", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-rag-8-10", "gemm", "bf16", 1, 0, 250, 130, 1024, 128, 128, PRED, 8, "8 slices, ragged tiles", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-rag-8-11", "gemm", "bf16", 1, 1, 250, 130, 1024, 128, 128, PRED, 8, "8 slices, ragged tiles", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-k131071-00", "gemm", "bf16", 0, 0, 64, 64, 131071, 128, 64, PRED, 256, "largest K with a = 8, ragged", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-k131071-10", "gemm", "bf16", 1, 0, 64, 64, 131071, 128, 64, PRED, 256, "largest K with a = 8, ragged", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-k262144-00", "gemm", "bf16", 0, 0, 32, 128, 262144, 32, 128, FAST, 256, "a = 4", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-k262144-10", "gemm", "bf16", 1, 0, 32, 128, 262144, 32, 128, FAST, 256, "a = 4", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-160-8tiles-00", "gemm", "bf16", 0, 0, 1024, 160, 512, 128, 160, FAST, 4, "128 x 160, 8 tiles", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-160-8tiles-01", "gemm", "bf16", 0, 1, 1024, 160, 512, 128, 160, FAST, 4, "128 x 160, 8 tiles", acc=(0, 1, 2), ldc_extra=4),
    C("bf16-cut-160-8tiles-10", "gemm", "bf16", 1, 0, 1024, 160, 512, 128, 160, FAST, 4, "128 x 160, 8 tiles", acc=(0, 1, 2), ldc_extra=0),
    C("bf16-cut-160-8tiles-11", "gemm", "bf16", 1, 1, 1024, 160, 512, 128, 160, FAST, 4, "128 x 160, 8 tiles", acc=(0, 1, 2), ldc_extra=4),
    # slice-ordered products: workspace full of NaN, C full of NaN, bias once
    C("f32-ordered-cut-00-bias", "ordered", "f32", 0, 0, 256, 128, 1024, 128, 128, FAST, 16, "ordered, cut", bias=True, ldc_extra=8),
    C("f32-ordered-cut-00-nobias", "ordered", "f32", 0, 0, 256, 128, 1024, 128, 128, FAST, 16, "ordered, cut", bias=False, ldc_extra=0),
    C("f32-ordered-cut-01-bias", "ordered", "f32", 0, 1, 256, 128, 1024, 128, 128, FAST, 16, "ordered, cut", bias=True, ldc_extra=8),
    C("f32-ordered-cut-01-nobias", "ordered", "f32", 0, 1, 256, 128, 1024, 128, 128, FAST, 16, "ordered, cut", bias=False, ldc_extra=0),
    C("f32-ordered-cut-10-bias", "ordered", "f32", 1, 0, 256, 128, 1024, 128, 128, FAST, 16, "ordered, cut", bias=True, ldc_extra=0),
    C("f32-ordered-cut-10-nobias", "ordered", "f32", 1, 0, 256, 128, 1024, 128, 128, FAST, 16, "ordered, cut", bias=False, ldc_extra=8),
    C("f32-ordered-cut-11-bias", "ordered", "f32", 1, 1, 256, 128, 1024, 128, 128, FAST, 16, "ordered, cut", bias=True, ldc_extra=0),
    C("f32-ordered-cut-11-nobias", "ordered", "f32", 1, 1, 256, 128, 1024, 128, 128, FAST, 16, "ordered, cut", bias=False, ldc_extra=8),
    C("f32-ordered-whole-00-bias", "ordered", "f32", 0, 0, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=True, ldc_extra=8),
    C("f32-ordered-whole-00-nobias", "ordered", "f32", 0, 0, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=False, ldc_extra=0),
    C("f32-ordered-whole-01-bias", "ordered", "f32", 0, 1, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=True, ldc_extra=8),
    C("f32-ordered-whole-01-nobias", "ordered", "f32", 0, 1, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=False, ldc_extra=0),
    C("f32-ordered-whole-10-bias", "ordered", "f32", 1, 0, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=True, ldc_extra=0),
    C("f32-ordered-whole-10-nobias", "ordered", "f32", 1, 0, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=False, ldc_extra=8),
    C("f32-ordered-whole-11-bias", "ordered", "f32", 1, 1, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=True, ldc_extra=0),
    C("f32-ordered-whole-11-nobias", "ordered", "f32", 1, 1, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=False, ldc_extra=8),
    C("f32-ordered-rag-cut-00-bias", "ordered", "f32", 0, 0, 250, 130, 1000, 128, 128, PRED, 8, "ordered, rag-cut", bias=True, ldc_extra=8),
    C("f32-ordered-rag-cut-00-nobias", "ordered", "f32", 0, 0, 250, 130, 1000, 128, 128, PRED, 8, "ordered, rag-cut", bias=False, ldc_extra=0),
    C("f32-ordered-rag-cut-01-bias", "ordered", "f32", 0, 1, 250, 130, 1000, 128, 128, PRED, 8, "ordered, rag-cut", bias=True, ldc_extra=8),
    C("f32-ordered-rag-cut-01-nobias", "ordered", "f32", 0, 1, 250, 130, 1000, 128, 128, PRED, 8, "ordered, rag-cut", bias=False, ldc_extra=0),
    C("f32-ordered-rag-cut-10-bias", "ordered", "f32", 1, 0, 250, 130, 1000, 128, 128, PRED, 8, "ordered, rag-cut", bias=True, ldc_extra=0),
    C("f32-ordered-rag-cut-10-nobias", "ordered", "f32", 1, 0, 250, 130, 1000, 128, 128, PRED, 8, "ordered, rag-cut", bias=False, ldc_extra=8),
    C("f32-ordered-rag-cut-11-bias", "ordered", "f32", 1, 1, 250, 130, 1000, 128, 128, PRED, 8, "ordered, rag-cut", bias=True, ldc_extra=0),
    C("f32-ordered-rag-cut-11-nobias", "ordered", "f32", 1, 1, 250, 130, 1000, 128, 128, PRED, 8, "ordered, rag-cut", bias=False, ldc_extra=8),
    C("bf16-ordered-cut-00-bias", "ordered", "bf16", 0, 0, 256, 128, 1024, 128, 128, FAST, 8, "ordered, cut", bias=True, ldc_extra=8),
    C("bf16-ordered-cut-00-nobias", "ordered", "bf16", 0, 0, 256, 128, 1024, 128, 128, FAST, 8, "ordered, cut", bias=False, ldc_extra=0),
    C("bf16-ordered-cut-01-bias", "ordered", "bf16", 0, 1, 256, 128, 1024, 128, 128, FAST, 8, "ordered, cut", bias=True, ldc_extra=8),
    C("bf16-ordered-cut-01-nobias", "ordered", "bf16", 0, 1, 256, 128, 1024, 128, 128, FAST, 8, "ordered, cut", bias=False, ldc_extra=0),
    C("bf16-ordered-cut-10-bias", "ordered", "bf16", 1, 0, 256, 128, 1024, 128, 128, FAST, 8, "ordered, cut", bias=True, ldc_extra=0),
    C("bf16-ordered-cut-10-nobias", "ordered", "bf16", 1, 0, 256, 128, 1024, 128, 128, FAST, 8, "ordered, cut", bias=False, ldc_extra=8),
    C("bf16-ordered-cut-11-bias", "ordered", "bf16", 1, 1, 256, 128, 1024, 128, 128, FAST, 8, "ordered, cut", bias=True, ldc_extra=0),
    C("bf16-ordered-cut-11-nobias", "ordered", "bf16", 1, 1, 256, 128, 1024, 128, 128, FAST, 8, "ordered, cut", bias=False, ldc_extra=8),
    C("bf16-ordered-whole-00-bias", "ordered", "bf16", 0, 0, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=True, ldc_extra=8),
    C("bf16-ordered-whole-00-nobias", "ordered", "bf16", 0, 0, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=False, ldc_extra=0),
    C("bf16-ordered-whole-01-bias", "ordered", "bf16", 0, 1, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=True, ldc_extra=8),
    C("bf16-ordered-whole-01-nobias", "ordered", "bf16", 0, 1, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=False, ldc_extra=0),
    C("bf16-ordered-whole-10-bias", "ordered", "bf16", 1, 0, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=True, ldc_extra=0),
    C("bf16-ordered-whole-10-nobias", "ordered", "bf16", 1, 0, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=False, ldc_extra=8),
    C("bf16-ordered-whole-11-bias", "ordered", "bf16", 1, 1, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=True, ldc_extra=0),
    C("bf16-ordered-whole-11-nobias", "ordered", "bf16", 1, 1, 256, 128, 64, 128, 128, FAST, 1, "ordered, whole", bias=False, ldc_extra=8),
    C("bf16-ordered-rag-cut-00-bias", "ordered", "bf16", 0, 0, 250, 130, 1000, 128, 128, PRED, 7, "ordered, rag-cut", bias=True, ldc_extra=8),
    C("bf16-ordered-rag-cut-00-nobias", "ordered", "bf16", 0, 0, 250, 130, 1000, 128, 128, PRED, 7, "ordered, rag-cut", bias=False, ldc_extra=0),
    C("bf16-ordered-rag-cut-01-bias", "ordered", "bf16", 0, 1, 250, 130, 1000, 128, 128, PRED, 7, "ordered, rag-cut", bias=True, ldc_extra=8),
    C("bf16-ordered-rag-cut-01-nobias", "ordered", "bf16", 0, 1, 250, 130, 1000, 128, 128, PRED, 7, "ordered, rag-cut", bias=False, ldc_extra=0),
    C("bf16-ordered-rag-cut-10-bias", "ordered", "bf16", 1, 0, 250, 130, 1000, 128, 128, PRED, 7, "ordered, rag-cut", bias=True, ldc_extra=0),
    C("bf16-ordered-rag-cut-10-nobias", "ordered", "bf16", 1, 0, 250, 130, 1000, 128, 128, PRED, 7, "ordered, rag-cut", bias=False, ldc_extra=8),
    C("bf16-ordered-rag-cut-11-bias", "ordered", "bf16", 1, 1, 250, 130, 1000, 128, 128, PRED, 7, "ordered, rag-cut", bias=True, ldc_extra=0),
    C("bf16-ordered-rag-cut-11-nobias", "ordered", "bf16", 1, 1, 250, 130, 1000, 128, 128, PRED, 7, "ordered, rag-cut", bias=False, ldc_extra=8),
    # cloudaae_gemm_f32_ordered_fold
    C("f32-ofold-dw-24-64", "ordered_fold", "f32", 1, 0, 24, 128, 4096, 32, 128, PRED, 64, "edge conv dW, cin 24 cout 64", fold_c=64),
    C("f32-ofold-dw-64-128", "ordered_fold", "f32", 1, 0, 64, 256, 4096, 64, 64, FAST, 64, "edge conv dW, cin 64 cout 128", fold_c=128),
    C("f32-ofold-dw-64-64", "ordered_fold", "f32", 1, 0, 64, 128, 4100, 64, 64, PRED, 52, "edge conv dW, ragged P", fold_c=64),
    C("f32-ofold-w64-x4", "ordered_fold", "f32", 1, 0, 64, 256, 4096, 64, 64, FAST, 64, "N / fold_c = 4", fold_c=64),
    C("f32-ofold-w128-x4", "ordered_fold", "f32", 0, 0, 24, 512, 2048, 32, 128, PRED, 32, "N / fold_c = 4, width 128", fold_c=128),
    C("f32-ofold-uncut", "ordered_fold", "f32", 1, 0, 64, 128, 64, 64, 64, FAST, 1, "stays whole: the kernel folds", fold_c=64),
    C("f32-ofold-nofold-cut", "ordered_fold", "f32", 1, 0, 64, 256, 4096, 64, 64, FAST, 64, "fold_c = 0", fold_c=0),
    C("f32-ofold-nofold-whole", "ordered_fold", "f32", 0, 1, 256, 128, 64, 128, 128, FAST, 1, "fold_c = 0, whole", fold_c=0),
    # column statistics
    C("f32-colstats-whole", "colstats", "f32", 0, 0, 512, 128, 64, 128, 128, FAST, 1, "whole tiles", ldc_extra=0),
    C("f32-colstats-ragrow", "colstats", "f32", 0, 0, 500, 128, 64, 128, 128, PRED, 1, "ragged last row tile", ldc_extra=0),
    C("f32-colstats-ragcol", "colstats", "f32", 0, 0, 512, 130, 64, 128, 128, PRED, 1, "ragged last column tile", ldc_extra=0),
    C("f32-colstats-rag-t", "colstats", "f32", 1, 1, 500, 130, 70, 128, 128, PRED, 1, "ragged, transposed", ldc_extra=4),
    C("f32-colstats-64rows", "colstats", "f32", 0, 1, 320, 128, 64, 64, 128, FAST, 1, "64-row tiles", ldc_extra=0),
    C("f32-colstats-m1", "colstats", "f32", 0, 0, 1, 128, 64, 32, 128, PRED, 1, "one row", ldc_extra=0),
    C("f32-colstats-160", "colstats", "f32", 0, 0, 1030, 160, 64, 64, 128, PRED, 1, "160-wide", ldc_extra=0),
    C("bf16-colstats-whole", "colstats", "bf16", 0, 0, 512, 128, 64, 128, 128, FAST, 1, "whole tiles", ldc_extra=0),
    C("bf16-colstats-ragrow", "colstats", "bf16", 0, 0, 500, 128, 64, 128, 128, PRED, 1, "ragged last row tile", ldc_extra=0),
    C("bf16-colstats-ragcol", "colstats", "bf16", 0, 0, 512, 130, 64, 128, 128, PRED, 1, "ragged last column tile", ldc_extra=0),
    C("bf16-colstats-rag-t", "colstats", "bf16", 1, 1, 500, 130, 70, 128, 128, PRED, 1, "ragged, transposed", ldc_extra=4),
    C("bf16-colstats-64rows", "colstats", "bf16", 0, 1, 320, 128, 64, 64, 128, FAST, 1, "64-row tiles", ldc_extra=0),
    C("bf16-colstats-m1", "colstats", "bf16", 0, 0, 1, 128, 64, 32, 128, PRED, 1, "one row", ldc_extra=0),
    C("bf16-colstats-160", "colstats", "bf16", 0, 0, 1030, 160, 64, 128, 160, PRED, 1, "160-wide", ldc_extra=0),
    # folded operands through cloudaae_dev_gemm_folded: the three products of edgeconv.hip
    C("f32-fold-c24-o64-p256-pq", "folded", "f32", 0, 0, 256, 128, 24, 128, 128, PRED, 1, "P|Q = x [Wc | Wn]", fold_b=64),
    C("f32-fold-c24-o64-p256-dx", "folded", "f32", 0, 1, 256, 24, 128, 128, 64, PRED, 2, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=64),
    C("f32-fold-c24-o64-p256-dw", "folded", "f32", 1, 0, 24, 128, 256, 32, 128, PRED, 4, "dW = x^T dpq, folded output", fold_c=64, acc=(0, 1, 2)),
    C("f32-fold-c24-o64-p250-pq", "folded", "f32", 0, 0, 250, 128, 24, 128, 128, PRED, 1, "P|Q = x [Wc | Wn]", fold_b=64),
    C("f32-fold-c24-o64-p250-dx", "folded", "f32", 0, 1, 250, 24, 128, 128, 64, PRED, 2, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=64),
    C("f32-fold-c24-o64-p250-dw", "folded", "f32", 1, 0, 24, 128, 250, 32, 128, PRED, 3, "dW = x^T dpq, folded output", fold_c=64, acc=(0, 1, 2)),
    C("f32-fold-c24-o128-p256-pq", "folded", "f32", 0, 0, 256, 256, 24, 128, 128, PRED, 1, "P|Q = x [Wc | Wn]", fold_b=128),
    C("f32-fold-c24-o128-p256-dx", "folded", "f32", 0, 1, 256, 24, 256, 128, 64, PRED, 4, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=128),
    C("f32-fold-c24-o128-p256-dw", "folded", "f32", 1, 0, 24, 256, 256, 32, 128, PRED, 4, "dW = x^T dpq, folded output", fold_c=128, acc=(0, 1, 2)),
    C("f32-fold-c24-o128-p250-pq", "folded", "f32", 0, 0, 250, 256, 24, 128, 128, PRED, 1, "P|Q = x [Wc | Wn]", fold_b=128),
    C("f32-fold-c24-o128-p250-dx", "folded", "f32", 0, 1, 250, 24, 256, 128, 64, PRED, 4, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=128),
    C("f32-fold-c24-o128-p250-dw", "folded", "f32", 1, 0, 24, 256, 250, 32, 128, PRED, 3, "dW = x^T dpq, folded output", fold_c=128, acc=(0, 1, 2)),
    C("f32-fold-c64-o64-p256-pq", "folded", "f32", 0, 0, 256, 128, 64, 128, 128, FAST, 1, "P|Q = x [Wc | Wn]", fold_b=64),
    C("f32-fold-c64-o64-p256-dx", "folded", "f32", 0, 1, 256, 64, 128, 128, 64, FAST, 2, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=64),
    C("f32-fold-c64-o64-p256-dw", "folded", "f32", 1, 0, 64, 128, 256, 64, 64, FAST, 4, "dW = x^T dpq, folded output", fold_c=64, acc=(0, 1, 2)),
    C("f32-fold-c64-o64-p250-pq", "folded", "f32", 0, 0, 250, 128, 64, 128, 128, PRED, 1, "P|Q = x [Wc | Wn]", fold_b=64),
    C("f32-fold-c64-o64-p250-dx", "folded", "f32", 0, 1, 250, 64, 128, 128, 64, PRED, 2, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=64),
    C("f32-fold-c64-o64-p250-dw", "folded", "f32", 1, 0, 64, 128, 250, 64, 64, PRED, 3, "dW = x^T dpq, folded output", fold_c=64, acc=(0, 1, 2)),
    C("f32-fold-c64-o128-p256-pq", "folded", "f32", 0, 0, 256, 256, 64, 128, 128, FAST, 1, "P|Q = x [Wc | Wn]", fold_b=128),
    C("f32-fold-c64-o128-p256-dx", "folded", "f32", 0, 1, 256, 64, 256, 128, 64, FAST, 4, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=128),
    C("f32-fold-c64-o128-p256-dw", "folded", "f32", 1, 0, 64, 256, 256, 64, 64, FAST, 4, "dW = x^T dpq, folded output", fold_c=128, acc=(0, 1, 2)),
    C("f32-fold-c64-o128-p250-pq", "folded", "f32", 0, 0, 250, 256, 64, 128, 128, PRED, 1, "P|Q = x [Wc | Wn]", fold_b=128),
    C("f32-fold-c64-o128-p250-dx", "folded", "f32", 0, 1, 250, 64, 256, 128, 64, PRED, 4, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=128),
    C("f32-fold-c64-o128-p250-dw", "folded", "f32", 1, 0, 64, 256, 250, 64, 64, PRED, 3, "dW = x^T dpq, folded output", fold_c=128, acc=(0, 1, 2)),
    C("f32-fold-dw-p4096", "folded", "f32", 1, 0, 64, 128, 4096, 64, 64, FAST, 64, "dW cut deep, folded atomics", fold_c=64, acc=(0, 1, 2)),
    C("f32-fold-both", "folded", "f32", 0, 0, 256, 128, 64, 128, 128, FAST, 1, "fold_b and fold_c together", fold_c=32, acc=(0, 1), fold_b=64),
    C("f32-fold-both-t", "folded", "f32", 0, 1, 250, 128, 128, 128, 128, PRED, 2, "fold_b over k and fold_c, ragged", fold_c=64, acc=(0, 1), fold_b=32),
    C("bf16-fold-c24-o64-p256-pq", "folded", "bf16", 0, 0, 256, 128, 24, 128, 128, PRED, 1, "P|Q = x [Wc | Wn]", fold_b=64),
    C("bf16-fold-c24-o64-p256-dx", "folded", "bf16", 0, 1, 256, 24, 128, 128, 64, PRED, 1, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=64),
    C("bf16-fold-c24-o64-p256-dw", "folded", "bf16", 1, 0, 24, 128, 256, 32, 128, PRED, 2, "dW = x^T dpq, folded output", fold_c=64, acc=(0, 1, 2)),
    C("bf16-fold-c24-o64-p250-pq", "folded", "bf16", 0, 0, 250, 128, 24, 128, 128, PRED, 1, "P|Q = x [Wc | Wn]", fold_b=64),
    C("bf16-fold-c24-o64-p250-dx", "folded", "bf16", 0, 1, 250, 24, 128, 128, 64, PRED, 1, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=64),
    C("bf16-fold-c24-o64-p250-dw", "folded", "bf16", 1, 0, 24, 128, 250, 32, 128, PRED, 1, "dW = x^T dpq, folded output", fold_c=64, acc=(0, 1, 2)),
    C("bf16-fold-c24-o128-p256-pq", "folded", "bf16", 0, 0, 256, 256, 24, 128, 128, PRED, 1, "P|Q = x [Wc | Wn]", fold_b=128),
    C("bf16-fold-c24-o128-p256-dx", "folded", "bf16", 0, 1, 256, 24, 256, 128, 64, PRED, 2, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=128),
    C("bf16-fold-c24-o128-p256-dw", "folded", "bf16", 1, 0, 24, 256, 256, 32, 128, PRED, 2, "dW = x^T dpq, folded output", fold_c=128, acc=(0, 1, 2)),
    C("bf16-fold-c24-o128-p250-pq", "folded", "bf16", 0, 0, 250, 256, 24, 128, 128, PRED, 1, "P|Q = x [Wc | Wn]", fold_b=128),
    C("bf16-fold-c24-o128-p250-dx", "folded", "bf16", 0, 1, 250, 24, 256, 128, 64, PRED, 2, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=128),
    C("bf16-fold-c24-o128-p250-dw", "folded", "bf16", 1, 0, 24, 256, 250, 32, 128, PRED, 1, "dW = x^T dpq, folded output", fold_c=128, acc=(0, 1, 2)),
    C("bf16-fold-c64-o64-p256-pq", "folded", "bf16", 0, 0, 256, 128, 64, 128, 128, FAST, 1, "P|Q = x [Wc | Wn]", fold_b=64),
    C("bf16-fold-c64-o64-p256-dx", "folded", "bf16", 0, 1, 256, 64, 128, 128, 64, FAST, 1, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=64),
    C("bf16-fold-c64-o64-p256-dw", "folded", "bf16", 1, 0, 64, 128, 256, 64, 128, FAST, 2, "dW = x^T dpq, folded output", fold_c=64, acc=(0, 1, 2)),
    C("bf16-fold-c64-o64-p250-pq", "folded", "bf16", 0, 0, 250, 128, 64, 128, 128, PRED, 1, "P|Q = x [Wc | Wn]", fold_b=64),
    C("bf16-fold-c64-o64-p250-dx", "folded", "bf16", 0, 1, 250, 64, 128, 128, 64, PRED, 1, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=64),
    C("bf16-fold-c64-o64-p250-dw", "folded", "bf16", 1, 0, 64, 128, 250, 64, 128, PRED, 1, "dW = x^T dpq, folded output", fold_c=64, acc=(0, 1, 2)),
    C("bf16-fold-c64-o128-p256-pq", "folded", "bf16", 0, 0, 256, 256, 64, 128, 128, FAST, 1, "P|Q = x [Wc | Wn]", fold_b=128),
    C("bf16-fold-c64-o128-p256-dx", "folded", "bf16", 0, 1, 256, 64, 256, 128, 64, FAST, 2, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=128),
    C("bf16-fold-c64-o128-p256-dw", "folded", "bf16", 1, 0, 64, 256, 256, 64, 128, FAST, 2, "dW = x^T dpq, folded output", fold_c=128, acc=(0, 1, 2)),
    C("bf16-fold-c64-o128-p250-pq", "folded", "bf16", 0, 0, 250, 256, 64, 128, 128, PRED, 1, "P|Q = x [Wc | Wn]", fold_b=128),
    C("bf16-fold-c64-o128-p250-dx", "folded", "bf16", 0, 1, 250, 64, 256, 128, 64, PRED, 2, "dx = dpq [Wc | Wn]^T", acc=(0, 1), fold_b=128),
    C("bf16-fold-c64-o128-p250-dw", "folded", "bf16", 1, 0, 64, 256, 250, 64, 128, PRED, 1, "dW = x^T dpq, folded output", fold_c=128, acc=(0, 1, 2)),
    C("bf16-fold-dw-p4096", "folded", "bf16", 1, 0, 64, 128, 4096, 64, 128, FAST, 32, "dW cut deep, folded atomics", fold_c=64, acc=(0, 1, 2)),
    C("bf16-fold-both", "folded", "bf16", 0, 0, 256, 128, 64, 128, 128, FAST, 1, "fold_b and fold_c together", fold_c=32, acc=(0, 1), fold_b=64),
    C("bf16-fold-both-t", "folded", "bf16", 0, 1, 250, 128, 128, 128, 128, PRED, 1, "fold_b over k and fold_c, ragged", fold_c=64, acc=(0, 1), fold_b=32),
    C("bf16-fold-b16-kc", "folded", "bf16", 0, 1, 256, 64, 64, 128, 64, PRED, 1, "fold width 16 < slab: must leave the predicate-free kernel", fold_b=16),
    C("f32-fold-b16-kc", "folded", "f32", 0, 1, 256, 64, 64, 128, 64, FAST, 1, "fold width 16: fp32 slabs are 16 deep", fold_b=16),
]

# cloudaae_gemm_b16 / cloudaae_gemm_bf16x3 / cloudaae_gemm_bf16x3p: tiles of 128 and 160 on both sides, the served transposes, a
# cut and an uncut K (K >= 512 / 256 cuts an output of few tiles; the slice counts are derived by hand from gemm_b16_plan and
# gemm_x3_plan: those files have no _splits query), accumulate as their header offers it, bf16 output where K stays whole.
OTHER = [
    C("b16-nn-128x128", "b16", "b16", 0, 0, 128, 128, 64, 128, 128, FAST, 1, "uncut", acc=(0, 1), c16=True),
    C("b16-nn-cut", "b16", "b16", 0, 0, 256, 256, 1024, 128, 128, FAST, 4, "four tiles, cut", acc=(0, 1), ldc_extra=8),
    C("b16-nt-128x160", "b16", "b16", 0, 1, 128, 160, 64, 128, 160, FAST, 1, "160-wide N", acc=(0, 1), c16=True, ldc_extra=8),
    C("b16-nt-128x128", "b16", "b16", 0, 1, 256, 128, 128, 128, 128, FAST, 1, "uncut", acc=(0, 1), c16=True, lda_extra=8),
    C("b16-nt-160-cut", "b16", "b16", 0, 1, 128, 320, 1024, 128, 160, FAST, 4, "160-wide N, cut", acc=(0, 1)),
    C("b16-tn-160x128", "b16", "b16", 1, 0, 160, 128, 64, 160, 128, FAST, 1, "160-wide M", acc=(0, 1), c16=True),
    C("b16-tn-128x128", "b16", "b16", 1, 0, 128, 256, 192, 128, 128, FAST, 1, "uncut", acc=(0, 1), c16=True, ldb_extra=8),
    C("b16-tn-160-cut", "b16", "b16", 1, 0, 320, 128, 8192, 160, 128, FAST, 32, "160-wide M, cut deep", acc=(0, 1), ldc_extra=4),
    C("b16-tt-refused", "b16", "b16", 1, 1, 128, 128, 64, 0, 0, None, 0, "both transposed: not served", refused=True),
    C("x3-nn-128x128", "bf16x3", "x3", 0, 0, 128, 128, 32, 128, 128, FAST, 1, "uncut", acc=(0, 1, 2)),
    C("x3-nn-cut", "bf16x3", "x3", 0, 0, 128, 128, 1024, 128, 128, FAST, 8, "one tile, cut", acc=(0, 1, 2), ldc_extra=4),
    C("x3-nn-streamed", "bf16x3", "x3", 0, 0, 24576, 128, 32, 128, 128, FAST, 1, "192 row tiles: the streamed route", acc=(0, 1, 2)),
    C("x3-nt-128x160", "bf16x3", "x3", 0, 1, 128, 160, 32, 128, 160, FAST, 1, "160-wide N", acc=(0, 1, 2), ldc_extra=4),
    C("x3-nt-128x128", "bf16x3", "x3", 0, 1, 256, 128, 64, 128, 128, FAST, 1, "uncut", acc=(0, 1, 2), lda_extra=4),
    C("x3-nt-160-cut", "bf16x3", "x3", 0, 1, 128, 320, 512, 128, 160, FAST, 4, "160-wide N, cut", acc=(0, 1, 2)),
    C("x3-tn-160x128", "bf16x3", "x3", 1, 0, 160, 128, 32, 160, 128, FAST, 1, "160-wide M", acc=(0, 1, 2)),
    C("x3-tn-128x128", "bf16x3", "x3", 1, 0, 128, 256, 96, 128, 128, FAST, 1, "uncut", acc=(0, 1, 2), ldb_extra=4),
    C("x3-tn-160-cut", "bf16x3", "x3", 1, 0, 320, 128, 8192, 160, 128, FAST, 64, "160-wide M, cut deep", acc=(0, 1, 2)),
    C("x3-tt-refused", "bf16x3", "x3", 1, 1, 128, 128, 32, 0, 0, None, 0, "both transposed: not served", refused=True),
    C("x3p-128x128", "bf16x3p", "x3p", 0, 1, 128, 128, 32, 128, 128, FAST, 1, "one tile", acc=(0, 1, 2)),
    C("x3p-128x160", "bf16x3p", "x3p", 0, 1, 128, 160, 32, 128, 160, FAST, 1, "160-wide N", acc=(0, 1, 2), ldc_extra=4),
    C("x3p-k96", "bf16x3p", "x3p", 0, 1, 256, 320, 96, 128, 160, FAST, 1, "three slabs", acc=(0, 1, 2), lda_extra=4),
    C("x3p-256rows", "bf16x3p", "x3p", 0, 1, 131072, 128, 32, 256, 128, FAST, 1, "512 tiles of 256 rows", acc=(0, 1)),
    C("x3p-refused", "bf16x3p", "x3p", 0, 1, 100, 128, 32, 0, 0, None, 0, "M not a multiple of 128: not served", refused=True),
]

SENTINEL = 777.0
GUARD_ROWS = 8


def kernel_variants(cases=None):
    """the (family, BM, BN, WM, WN, TA, TB, FAST) the rows of CASES claim to reach in gemm.hip / gemm_bf16.hip"""
    return sorted(set((c.fam, c.BM, c.BN) + WAVES[(c.BM, c.BN)] + (bool(c.ta), bool(c.tb), c.fast)
                      for c in (CASES if cases is None else cases)))


def check_claims(case, cdll, set_knob):
    """What the library's queries can confirm of a row: its K slices, and BM as the tile rows of the uncut product
    (CLOUDAAE_DETERMINISTIC keeps a product whole, with its tile shape).  Host arithmetic: needs no GPU."""
    M, N, K = case.M, case.N, case.K
    if case.fam in ("f32", "bf16"):
        assert getattr(cdll, "cloudaae_gemm_%s_splits" % case.fam)(M, N, K) == case.slices, case.id
        if case.entry in ("ordered", "ordered_fold"):
            need = getattr(cdll, "cloudaae_gemm_%s_ordered_workspace" % case.fam)(M, N, K)
            assert need == (case.slices * M * N if case.slices > 1 else 0), case.id
        if case.slices > 1:
            set_knob("CLOUDAAE_DETERMINISTIC", 1)
        try:
            parts = getattr(cdll, "cloudaae_gemm_%s_colstats_parts" % case.fam)(M, N, K)
        finally:
            if case.slices > 1:
                set_knob("CLOUDAAE_DETERMINISTIC", None)
        assert parts == -(-M // case.BM), (case.id, parts)
        return
    q = {"b16": lambda: cdll.cloudaae_gemm_b16_supported(case.ta, case.tb, M, N, K),
         "x3": lambda: cdll.cloudaae_gemm_bf16x3_supported(case.ta, case.tb, M, N, K),
         "x3p": lambda: cdll.cloudaae_gemm_bf16x3p_supported(M, N, K)}[case.fam]()
    assert q == (0 if case.opts.get("refused") else 1), case.id


def amplitude(K):
    """the largest a in {8, 4, 2, 1} with 2 K a^2 + 2 a < 2^24: every partial sum of a product of such integers, plus the bias,
    plus a prior C of that size, is an integer fp32 holds exactly"""
    a = 8
    while a > 1 and 2 * K * a * a + 2 * a >= 2 ** 24:
        a //= 2
    assert 2 * K * a * a + 2 * a < 2 ** 24, K
    return a


def _ints(shape, a, gen):
    """non-zero integers in [-a, a], random signs, float32 on the GPU"""
    mag = torch.randint(1, a + 1, shape, generator=gen, device="cuda")
    sign = torch.randint(0, 2, shape, generator=gen, device="cuda") * 2 - 1
    return (mag * sign).float()


def _up4(n):
    return (n + 3) // 4 * 4


PAD = 64        # elements before and after an operand inside its NaN-filled buffer (a multiple of 16 bytes for both types)


def _place(mat, ld, off=0, dtype=torch.float32):
    """mat [rows, cols] with leading dimension ld inside a NaN-filled buffer, `off` elements past a 16-byte aligned address
    -> (buffer, device address of element (0, 0))"""
    rows, cols = mat.shape
    assert ld >= cols
    buf = torch.full((PAD + off + rows * ld + PAD,), float("nan"), dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[PAD + off:PAD + off + rows * ld].view(rows, ld)[:, :cols] = mat.to(dtype)
    return buf, buf.data_ptr() + buf.element_size() * (PAD + off)


def fold_index(rows, cols, width):
    """gemm.h's Fold: logical (r, c) of a [rows, cols] matrix lives at physical row (c >> shift) * rows + r, column
    c & (width - 1) of a [ceil(cols / width) * rows, width] matrix -> (physical rows, row index [rows, cols], column index)"""
    shift = int(math.log2(width))
    assert 1 << shift == width
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    prow = (c >> shift) * rows + r
    pcol = (c & (width - 1)) + 0 * r
    return -(-cols // width) * rows, torch.from_numpy(prow).cuda(), torch.from_numpy(pcol).cuda()


def _folded(mat, width):
    """the folded storage of logical `mat` (NaN where no logical element lives)"""
    prows, prow, pcol = fold_index(mat.shape[0], mat.shape[1], width)
    phys = torch.full((prows, width), float("nan"), dtype=mat.dtype, device="cuda")
    phys[prow, pcol] = mat
    return phys


class Out(object):
    """An output [rows, cols] with leading dimension ld >= cols inside guard rows and columns that hold SENTINEL."""

    def __init__(self, rows, cols, ld, prior, dtype=torch.float32):
        self.rows, self.cols = rows, cols
        self.buf = torch.full((GUARD_ROWS + rows + GUARD_ROWS, ld), SENTINEL, dtype=dtype, device="cuda")
        self.block = self.buf[GUARD_ROWS:GUARD_ROWS + rows, :cols]
        self.block.copy_(prior)
        self.ptr = self.buf.data_ptr() + self.buf.element_size() * GUARD_ROWS * ld

    def guards_intact(self):
        bits = self.buf.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[self.buf.element_size()])
        want = torch.full((1,), SENTINEL, dtype=self.buf.dtype, device="cuda").view(bits.dtype)
        g = GUARD_ROWS
        return bool((bits[:g] == want).all() and (bits[g + self.rows:] == want).all() and
                    (bits[g:g + self.rows, self.cols:] == want).all())


def _operands(case, gen, dtype=torch.float32):
    """-> a, (A buffer, address, lda), (B buffer, address, ldb), bias, the float64 product op(A) op(B) [M, N]"""
    M, N, K, o = case.M, case.N, case.K, case.opts
    a = amplitude(K)
    A = _ints((K, M) if case.ta else (M, K), a, gen)
    B = _ints((N, K) if case.tb else (K, N), a, gen)
    want = (A.t() if case.ta else A).double() @ (B.t() if case.tb else B).double()
    assert float(want.abs().max()) <= K * a * a
    lda = _up4(A.shape[1]) + o.get("lda_extra", 0)
    Bs, ldb = B, _up4(B.shape[1]) + o.get("ldb_extra", 0)
    if o.get("fold_b"):
        Bs, ldb = _folded(B, o["fold_b"]), o["fold_b"]
    bufA, pA = _place(A, lda, o.get("a_off", 0), dtype)
    bufB, pB = _place(Bs, ldb, o.get("b_off", 0), dtype)
    bias = _ints((N,), a, gen)
    return a, (bufA, pA, lda), (bufB, pB, ldb), bias, want


def _prior(acc, shape, a, gen):
    if acc == 0:
        return torch.full(shape, float("nan"), device="cuda")
    return _ints(shape, a, gen) if acc == 1 else torch.zeros(shape, device="cuda")


def _expect(want, bias, prior, acc, fold_c):
    """the exact fp32 result in the output's storage: (prior +) product (+ bias), folded like the output"""
    e = want + (bias.double() if bias is not None else 0.0)
    e = e.float()
    assert torch.equal(e.double(), want + (bias.double() if bias is not None else 0.0))
    if fold_c:
        e = _folded(e, fold_c)
    return prior + e if acc == 1 else e


def _launch(hip, case, acc, A, B, out, ldc, bias, extra):
    L, s = hip.lib(), hip.stream()
    M, N, K, ta, tb = case.M, case.N, case.K, case.ta, case.tb
    pb = bias.data_ptr() if bias is not None else None
    fb, fc = case.opts.get("fold_b", 0), case.opts.get("fold_c", 0)
    head = (ta, tb, M, N, K, A[1], A[2], B[1], B[2], out.ptr, ldc)
    if case.entry == "gemm":
        return getattr(L, "cloudaae_gemm_" + case.fam)(*head, pb, acc, s)
    if case.entry == "ordered":
        return getattr(L, "cloudaae_gemm_%s_ordered" % case.fam)(*head, pb, extra[0], extra[1], s)
    if case.entry == "ordered_fold":
        return L.cloudaae_gemm_f32_ordered_fold(*head, fc, extra[0], extra[1], s)
    if case.entry == "colstats":
        return getattr(L, "cloudaae_gemm_%s_colstats" % case.fam)(*head, pb, extra, s)
    if case.entry == "folded":
        return L.cloudaae_dev_gemm_folded(1 if case.fam == "bf16" else 0, *head, acc, fb, fc, s)
    raise AssertionError(case.entry)


def run_case(hip, knobs, case):
    """Draws the operands, places C inside its guards, calls the entry point once per accumulate mode and demands the bits of
    the integer product in the logical block and untouched guards."""
    L = hip.lib()
    check_claims(case, L._cdll, knobs)
    M, N, K, o = case.M, case.N, case.K, case.opts
    gen = torch.Generator(device="cuda").manual_seed(abs(hash((M, N, K, case.ta, case.tb))) % (2 ** 31))
    a, A, B, bias, want = _operands(case, gen)
    takes_bias = case.entry in ("gemm", "ordered", "colstats")
    if not (takes_bias and o.get("bias", True)):
        bias = None
    fc = o.get("fold_c", 0)
    rows, cols = (-(-N // fc) * M, fc) if fc else (M, N)
    ldc = fc if fc else _up4(N) + o.get("ldc_extra", 0)
    for acc in o.get("acc", (0,)):
        prior = _prior(acc, (rows, cols), a, gen)
        out = Out(rows, cols, ldc, prior)
        extra = ws = cs = None
        if case.entry in ("ordered", "ordered_fold"):
            n = int(getattr(L, "cloudaae_gemm_%s_ordered_workspace" % case.fam)(M, N, K))
            ws = Out(1, max(n, 4), max(n, 4), torch.full((1, max(n, 4)), float("nan"), device="cuda"))
            extra = (ws.ptr if n else None, n)
        elif case.entry == "colstats":
            parts = int(getattr(L, "cloudaae_gemm_%s_colstats_parts" % case.fam)(M, N, K))
            assert parts == -(-M // case.BM) and parts > 0
            cs = Out(1, parts * 2 * N, parts * 2 * N + 16, torch.full((1, parts * 2 * N), float("nan"), dtype=torch.float64,
                                                                       device="cuda"), dtype=torch.float64)
            extra = cs.ptr
        hip.check(_launch(hip, case, acc, A, B, out, ldc, bias, extra), case.id)
        torch.cuda.synchronize()
        expect = _expect(want, bias, prior, acc, fc)
        same = torch.eq(out.block, expect) | (torch.isnan(expect) & torch.isnan(out.block))     # (NaN: no logical element there)
        assert bool(same.all()), "%s accumulate %d: %d of %d elements differ, first at %s" % (
            case.id, acc, int((~same).sum()), same.numel(), (~same).nonzero()[0].tolist())
        assert not fc or (N % fc == 0 and torch.equal(out.block, expect))
        assert out.guards_intact(), "%s accumulate %d: a guard element around C changed" % (case.id, acc)
        if ws is not None:
            assert ws.guards_intact(), case.id + ": a guard element around the workspace changed"
        if cs is not None:
            # fp64 sums of integers: exact while max|C|^2 * M < 2^53
            e = expect.double()
            assert float(e.abs().max()) ** 2 * M < 2 ** 53
            assert cs.guards_intact(), case.id + ": a guard element after the column statistics changed"
            got = cs.block.reshape(parts, 2, N)
            for p in range(parts):      # padding rows of the last tile must not enter the sums
                rows_p = e[p * case.BM:(p + 1) * case.BM]
                assert torch.equal(got[p, 0], rows_p.sum(0)) and torch.equal(got[p, 1], (rows_p * rows_p).sum(0)), (case.id, p)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gemm_exact(hip, knobs, case):
    run_case(hip, knobs, case)


def _x3_planes(hip, B_nk, N, K):
    """the three bfloat16 planes of the [N][K] operand (cloudaae_x3_split)"""
    L = hip.lib()
    assert L.cloudaae_x3_planes_bytes(N, K) == 6 * N * K
    planes = torch.full((3 * N * K + 16,), float("nan"), dtype=torch.bfloat16, device="cuda")
    src = B_nk.contiguous()
    hip.check(L.cloudaae_x3_split(N, K, src.data_ptr(), K, 0, planes.data_ptr(), hip.stream()), "x3_split")
    return planes


@pytest.mark.parametrize("case", OTHER, ids=[c.id for c in OTHER])
def test_gemm_exact_bf16_storage_and_split_products(hip, knobs, case):
    """cloudaae_gemm_b16 (operands that are bfloat16 in memory; fp32 or bfloat16 output), cloudaae_gemm_bf16x3 and
    cloudaae_gemm_bf16x3p, over shapes their _supported query accepts; one refused shape each must leave C untouched."""
    L, s = hip.lib(), hip.stream()
    check_claims(case, L._cdll, knobs)
    M, N, K, ta, tb, o = case.M, case.N, case.K, case.ta, case.tb, case.opts
    gen = torch.Generator(device="cuda").manual_seed(M + 3 * N + 7 * K + ta)
    b16 = case.entry == "b16"
    a, A, B, bias, want = _operands(case, gen, torch.bfloat16 if b16 else torch.float32)
    ldc = _up4(N) + o.get("ldc_extra", 0)
    planes = None
    if case.entry == "bf16x3p" and not o.get("refused"):
        planes = _x3_planes(hip, B[0][PAD:PAD + N * B[2]].view(N, B[2])[:, :K], N, K)

    def call(acc, out, c16=0):
        if b16:
            return L.cloudaae_gemm_b16(ta, tb, M, N, K, A[1], A[2], B[1], B[2], out.ptr, ldc, c16, bias.data_ptr(), acc, None, s)
        if case.entry == "bf16x3":
            return L.cloudaae_gemm_bf16x3(ta, tb, M, N, K, A[1], A[2], B[1], B[2], out.ptr, ldc, bias.data_ptr(), acc, None, s)
        return L.cloudaae_gemm_bf16x3p(M, N, K, A[1], A[2], planes.data_ptr() if planes is not None else B[1], out.ptr, ldc,
                                       bias.data_ptr(), acc, None, s)

    if o.get("refused"):
        out = Out(M, N, ldc, torch.full((M, N), SENTINEL, device="cuda"))
        assert call(0, out) != 0 and "not served" in L.cloudaae_last_error().decode()
        torch.cuda.synchronize()
        assert out.guards_intact() and bool((out.block == SENTINEL).all())
        return
    for acc in o.get("acc", (0,)):
        prior = _prior(acc, (M, N), a, gen)
        out = Out(M, N, ldc, prior)
        hip.check(call(acc, out), case.id)
        torch.cuda.synchronize()
        assert torch.equal(out.block, _expect(want, bias, prior, acc, 0)), "%s accumulate %d" % (case.id, acc)
        assert out.guards_intact(), "%s accumulate %d: a guard element around C changed" % (case.id, acc)
    if o.get("c16"):
        # a bfloat16 output is the round-to-nearest-even of the exact integer: what torch's .bfloat16() gives
        ldc16 = (N + 7) // 8 * 8 + 8
        out = Out(M, N, ldc16, torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda"), dtype=torch.bfloat16)
        hip.check(L.cloudaae_gemm_b16(ta, tb, M, N, K, A[1], A[2], B[1], B[2], out.ptr, ldc16, 1, bias.data_ptr(), 0, None, s),
                  case.id)
        torch.cuda.synchronize()
        assert torch.equal(out.block, _expect(want, bias, None, 0, 0).bfloat16()), case.id + " bf16 output"
        assert out.guards_intact(), case.id + ": a guard element around the bf16 C changed"


# cloudaae_gemm_f32_tn_group: every job runs gemm_f32_tile<64, 128> predicated with atomics (one kernel, no variants to claim).
# (M, N, K, fold_c, zeroed, lda - M): M = 24 / 130 and N = 70 are ragged; K < 512 stays whole (a slice gets >= 256 k), larger K cuts.
GROUPS = {
    "one": [(64, 128, 4096, 64, 1, 0)],
    "three": [(24, 128, 5000, 64, 1, 8), (130, 70, 777, 0, 0, 2), (64, 256, 300, 128, 0, 4)],
    "eight": [(24, 128, 5000, 64, 1, 8), (64, 128, 4096, 64, 0, 0), (64, 256, 32768, 128, 1, 4), (130, 70, 777, 0, 0, 6),
              (24, 128, 300, 0, 1, 0), (130, 256, 2048, 128, 0, 1), (64, 70, 4096, 0, 1, 4), (24, 512, 520, 128, 0, 8)],
}


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_gemm_tn_group_exact(hip, name):
    """1, 3 and 8 weight-gradient products C_j = A_j^T B_j in one launch: mixed shapes, plain and folded outputs, outputs cleared
    by the caller (zeros) and by the call (NaN before it), K that cuts and K that stays whole, lda > M, guards around every C_j."""
    L = hip.lib()
    shapes = GROUPS[name]
    jobs = (hip.GemmTnJob * len(shapes))()
    gen = torch.Generator(device="cuda").manual_seed(len(shapes))
    keep = []
    for j, (M, N, K, fold, zeroed, pad) in zip(jobs, shapes):
        a = amplitude(K)
        A, B = _ints((K, M), a, gen), _ints((K, N), a, gen)
        bufA, pA = _place(A, M + pad)
        bufB, pB = _place(B, _up4(N))
        rows, cols = ((N // fold) * M, fold) if fold else (M, N)
        ldc = fold if fold else _up4(N) + 4
        out = Out(rows, cols, ldc, torch.zeros(rows, cols, device="cuda") if zeroed else
                  torch.full((rows, cols), float("nan"), device="cuda"))
        j.M, j.N, j.K, j.A, j.lda, j.B, j.ldb, j.C, j.ldc, j.fold_c, j.zeroed = M, N, K, pA, M + pad, pB, _up4(N), out.ptr, ldc, fold, zeroed
        want = (A.double().t() @ B.double()).float()
        keep.append((bufA, bufB, out, _folded(want, fold) if fold else want))
    hip.check(L.cloudaae_gemm_f32_tn_group(len(shapes), jobs, hip.stream()), "tn_group")
    torch.cuda.synchronize()
    for shape, (_, _, out, want) in zip(shapes, keep):
        assert torch.equal(out.block, want), shape
        assert out.guards_intact(), shape
