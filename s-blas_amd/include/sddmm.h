// sddmm.h -- val(A)[e] = alpha * <X[row(e), :], Y[col(e), :]> + beta * val(A)[e] for every stored entry e of a CSR matrix A
// (sampled dense-dense matrix product: A gives the pattern and receives the values), on one or more MI355X.
//
//   sblas_sddmm_csr_cpu  single-threaded host loop (the verifier the driver compares against), writes pA->csrVal
//   sblas_sddmm_csr      A split into nnz-balanced row blocks, X and Y replicated: GPU i computes the values of its own
//                        nonzeros into csrVal_gpu[i] (X advanced to the block's first row).  The blocks are disjoint in
//                        nonzeros, so there is no merge and no communication; each block is copied back into pA->csrVal.
// X is height x k, Y is width x k, each column- or row-major.  The bits of a value depend on its two operand rows, k, alpha,
// beta and the old value alone (include/sblas_hip.h), so any number of GPUs gives the same bits.  <int, double> only: the
// reference's other type pairs have no SDDMM to be compatible with.
#ifndef SBLAS_AMD_SDDMM_H
#define SBLAS_AMD_SDDMM_H

#include <assert.h>
#include <iostream>
#include <type_traits>
#include <stdlib.h>

#include "matrix.h"
#include "utility.h"

using namespace std;

namespace sblas_detail {

template <typename IdxType, typename DataType> inline void require_int_double(const char *who)
{
    if (!(std::is_same<IdxType, int>::value && std::is_same<DataType, double>::value)) {
        cerr << who << ": only <int, double> is supported!" << endl;
        exit(-1);
    }
}

// element (r, j) of a dense operand on the host
template <typename IdxType, typename DataType>
inline DataType dense_at(const DenseMatrix<IdxType, DataType> *p, size_t r, size_t j)
{
    return p->order == row_major ? p->val[r * (size_t)p->width + j] : p->val[j * (size_t)p->height + r];
}

} // namespace sblas_detail

// Host verifier: a plain loop over the entries, the k products added in order.
template <typename IdxType, typename DataType>
void sblas_sddmm_csr_cpu(CsrSparseMatrix<IdxType, DataType> *pA, DenseMatrix<IdxType, DataType> *pX,
                         DenseMatrix<IdxType, DataType> *pY, DataType alpha, DataType beta)
{
    assert((pA->height) == (pX->height));
    assert((pA->width) == (pY->height));
    assert((pX->width) == (pY->width));
    const size_t M = (size_t)pA->height, K = (size_t)pX->width;
    for (size_t i = 0; i < M; ++i)
        for (IdxType e = pA->csrRowPtr[i]; e < pA->csrRowPtr[i + 1]; ++e) {
            const size_t c = (size_t)pA->csrColIdx[e];
            DataType sum = 0;
            for (size_t j = 0; j < K; ++j) sum += sblas_detail::dense_at(pX, i, j) * sblas_detail::dense_at(pY, c, j);
            pA->csrVal[e] = beta == (DataType)0 ? alpha * sum : beta * pA->csrVal[e] + alpha * sum;
        }
}

// Preconditions: A.sync2gpu(g, segment); X, Y .sync2gpu(g, replicate), either order each.  On return pA->csrVal and every
// csrVal_gpu[i] hold the new values (GPU i those of its own block).
template <typename IdxType, typename DataType>
void sblas_sddmm_csr(CsrSparseMatrix<IdxType, DataType> *pA, DenseMatrix<IdxType, DataType> *pX,
                     DenseMatrix<IdxType, DataType> *pY, DataType alpha, DataType beta, unsigned n_gpu)
{
    sblas_detail::require_int_double<IdxType, DataType>("SBLAS_SDDMM_CSR");
    assert((pA->height) == (pX->height));
    assert((pA->width) == (pY->height));
    assert((pX->width) == (pY->width));
    assert(pA->policy == segment && pX->policy == replicate && pY->policy == replicate);
    const int64_t M = pA->height, N = pA->width, K = pX->width;
    const int ox = pX->order == row_major ? SBLAS_ROW_MAJOR : SBLAS_COL_MAJOR;
    const int oy = pY->order == row_major ? SBLAS_ROW_MAJOR : SBLAS_COL_MAJOR;
    const int64_t ldx = ox == SBLAS_ROW_MAJOR ? K : M, ldy = oy == SBLAS_ROW_MAJOR ? K : N;
    for (unsigned i = 0; i < n_gpu; ++i) { // asynchronous: every GPU is busy before the first one finishes
        CUDA_SAFE_CALL(cudaSetDevice((int)i));
        const int64_t m_i = (int64_t)pA->get_gpu_row_ptr_num(i) - 1, nnz_i = (int64_t)pA->nnz_gpu[i];
        const int64_t start = (int64_t)pA->starting_row_gpu[i];
        int32_t s4 = 0, e4 = 0, k4 = 0;
        int64_t first = 0;
        if (sblas_partition_nnz((const int32_t *)pA->csrRowPtr, (int32_t)M, (int32_t)pA->nnz, (int)n_gpu, (int)i, &s4, &e4, &k4,
                                &first, NULL) < 0) {
            cerr << "SBLAS_SDDMM_CSR: cannot split the nonzeros over " << n_gpu << " GPUs" << endl;
            exit(-1);
        }
        // the block's rows of X: a row-major X advanced by whole rows, a column-major X by elements of its first column
        // (the leading dimension stays M, which is at least the block's row count)
        const double *X = (const double *)pX->val_gpu[i] + (ox == SBLAS_ROW_MAJOR ? (size_t)start * (size_t)K : (size_t)start);
        const size_t ws_bytes = sblas_hip_sddmm_csr_workspace(m_i, N, nnz_i, K, ox, oy);
        void *ws = ws_bytes ? sblas_rt::workspace(i, ws_bytes) : NULL;
        sblas_rt::must_sblas(sblas_hip_sddmm_csr_f64_i32(-1, sblas_rt::stream(i), m_i, N, nnz_i, (const int32_t *)pA->csrRowPtr_gpu[i],
                                                         (const int32_t *)pA->csrColIdx_gpu[i], X, ldx, ox,
                                                         (const double *)pY->val_gpu[i], ldy, oy, K, (double)alpha, (double)beta,
                                                         (double *)pA->csrVal_gpu[i], ws, ws_bytes),
                             "sblas_hip_sddmm_csr_f64_i32");
        if (nnz_i > 0)
            CUDA_SAFE_CALL(hipMemcpyAsync(pA->csrVal + first, pA->csrVal_gpu[i], (size_t)nnz_i * sizeof(DataType),
                                          hipMemcpyDeviceToHost, sblas_rt::stream(i)));
    }
    sblas_rt::sync_all(n_gpu);
    CUDA_CHECK_ERROR();
}

#endif
