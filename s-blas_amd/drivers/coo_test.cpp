// coo_test -- CSR from shuffled COO triplets: the file's entries are read as COO (no symmetric expansion), the
// off-diagonal entries of a symmetric file are mirrored, the triplets are shuffled with a fixed seed and
// CsrSparseMatrix(coo, dup) converts them on GPU 0 in both duplicate modes.  For a file without duplicates whose rows the
// loader leaves in ascending column order (ash85) both must equal CsrSparseMatrix(file) bit for bit; sblas_spmv_csr_v1
// then runs on all three and the results are compared with ==.   coo_test <matrix> <gpus>
#include <cstring>
#include <random>

#include "harness.h"

static bool same_csr(CsrSparseMatrix<int, double> &a, CsrSparseMatrix<int, double> &b, const char *what)
{
    const bool ok = a.height == b.height && a.width == b.width && a.nnz == b.nnz &&
                    !memcmp(a.csrRowPtr, b.csrRowPtr, a.get_row_ptr_size()) &&
                    !memcmp(a.csrColIdx, b.csrColIdx, a.get_col_idx_size()) && !memcmp(a.csrVal, b.csrVal, a.get_val_size());
    printf("%s: nnz %d, arrays %s\n", what, (int)b.nnz, ok ? "bit-identical" : "DIFFER");
    return ok;
}

int main(int argc, char *argv[])
{
    if (argc < 3) {
        cerr << "usage: coo_test <matrix.mtx> <gpus>" << endl;
        return 1;
    }
    const unsigned n_gpu = (unsigned)atoi(argv[2]);
    CsrSparseMatrix<int, double> A(argv[1]);
    if (A.height == 0 || A.nnz == 0 || n_gpu == 0) return 1;
    int m = 0, n = 0, nnz_full = 0, sym = 0;
    mmio_info(&m, &n, &nnz_full, &sym, argv[1]);
    CooSparseMatrix<int, double> file(argv[1]);
    CooSparseMatrix<int, double> coo;
    coo.height = file.height, coo.width = file.width;
    size_t total = (size_t)file.nnz;
    if (sym)
        for (size_t k = 0; k < (size_t)file.nnz; ++k) total += file.cooRowIdx[k] != file.cooColIdx[k];
    coo.nnz = (int)total;
    SAFE_ALOC_HOST(coo.cooRowIdx, coo.get_nnz_idx_size());
    SAFE_ALOC_HOST(coo.cooColIdx, coo.get_nnz_idx_size());
    SAFE_ALOC_HOST(coo.cooVal, coo.get_nnz_val_size());
    size_t w = 0;
    for (size_t k = 0; k < (size_t)file.nnz; ++k) {
        const int r = file.cooRowIdx[k], c = file.cooColIdx[k];
        coo.cooRowIdx[w] = r, coo.cooColIdx[w] = c, coo.cooVal[w] = file.cooVal[k], ++w;
        if (sym && r != c) coo.cooRowIdx[w] = c, coo.cooColIdx[w] = r, coo.cooVal[w] = file.cooVal[k], ++w;
    }
    std::mt19937 rng(RAND_INIT_SEED); // Fisher-Yates with a fixed seed
    for (size_t i = total; i > 1; --i) {
        const size_t j = rng() % i;
        std::swap(coo.cooRowIdx[i - 1], coo.cooRowIdx[j]);
        std::swap(coo.cooColIdx[i - 1], coo.cooColIdx[j]);
        std::swap(coo.cooVal[i - 1], coo.cooVal[j]);
    }
    CsrSparseMatrix<int, double> keep(coo, SBLAS_COO_KEEP), sum(coo, SBLAS_COO_SUM);
    bool ok = same_csr(A, keep, "keep") & same_csr(A, sum, "sum");

    DenseVector<int, double> x(A.width), y(A.height, 1.), y_keep(A.height, 1.), y_sum(A.height, 1.);
    A.sync2gpu(n_gpu, segment);
    keep.sync2gpu(n_gpu, segment);
    sum.sync2gpu(n_gpu, segment);
    x.sync2gpu(n_gpu, replicate);
    y.sync2gpu(n_gpu, replicate);
    y_keep.sync2gpu(n_gpu, replicate);
    y_sum.sync2gpu(n_gpu, replicate);
    sblas_spmv_csr_v1<int, double>(&A, &x, &y, 3.0, 0.5, n_gpu);
    sblas_spmv_csr_v1<int, double>(&keep, &x, &y_keep, 3.0, 0.5, n_gpu);
    sblas_spmv_csr_v1<int, double>(&sum, &x, &y_sum, 3.0, 0.5, n_gpu);
    CUDA_CHECK_ERROR();
    y.sync2cpu(0);
    y_keep.sync2cpu(0);
    y_sum.sync2cpu(0);
    bool spmv = true;
    for (size_t i = 0; i < y.get_vec_length(); ++i) spmv = spmv && y.val[i] == y_keep.val[i] && y.val[i] == y_sum.val[i];
    printf("spmv on %u GPU(s): %s\n", n_gpu, spmv ? "equal" : "DIFFERS");
    ok = ok && spmv;
    cout << "coo_test: " << (ok ? "PASS" : "FAIL") << endl;
    return ok ? 0 : 2;
}
