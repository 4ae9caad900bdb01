// Block sizes of the blocked dense algorithms (Cholesky forward / reverse,
// triangular solves, LU, the MVN paths) and the layout of the Cholesky aux
// buffer.  Constants only: the 64 x 64 block code itself is tri_small.h.
#pragma once

constexpr int SMG_NB = 64;           // diagonal block size of every blocked kernel
constexpr int SMG_NBR = 512;         // outer block of the two-level Cholesky reverse
#ifndef SMG_NBF_COLS
#define SMG_NBF_COLS 512
#endif
constexpr int SMG_NBF = SMG_NBF_COLS;  // panel width of the two-level Cholesky forward
// cholesky aux layout (n rows each, ld n): inverses of the 64-, 128-, 256-
// and 512-row diagonal blocks of L
constexpr int SMG_AUX_W128 = SMG_NB;
constexpr int SMG_AUX_W256 = SMG_NB + 128;
constexpr int SMG_AUX_W512 = SMG_NB + 128 + 256;
constexpr int SMG_AUX_COLS = SMG_NB + 128 + 256 + 512;
constexpr int SMG_NBP = SMG_NB + 1;  // padded LDS row stride
constexpr int SMG_DIAG_THREADS = 512;  // threads of the fused diagonal-block kernels
