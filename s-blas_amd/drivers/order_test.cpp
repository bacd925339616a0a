// order_test -- method 2 with row-major B and C: sblas_spmm_csr_v2 on column-major B / C and on their row-major twins
// (DenseMatrix::transpose), each called twice (the second call runs on the per-GPU plans).  The column-major result must
// match the host verifier, and the row-major result must be its transpose bit for bit (same kernels, same order of the
// terms; only the staging copy and the write-back see the layout).   order_test <matrix> <B_width> <gpus>
// (SBLAS_MERGE=allreduce selects the reference's merge; with a column-major C and 256+ columns the column-tile pipeline
// runs, which a row-major C never takes.)
#include <cstring>

#include "harness.h"

int main(int argc, char *argv[])
{
    if (argc < 4) {
        cerr << "usage: order_test <matrix.mtx> <B_width> <gpus>" << endl;
        return 1;
    }
    const int b_width = atoi(argv[2]);
    const unsigned n_gpu = (unsigned)atoi(argv[3]);
    CsrSparseMatrix<int, double> A(argv[1]);
    if (A.height == 0 || A.nnz == 0 || b_width <= 0 || n_gpu == 0) return 1;
    DenseMatrix<int, double> B(A.width, b_width, col_major);
    DenseMatrix<int, double> C(A.height, b_width, 1.0, col_major), C_cpu(A.height, b_width, 1.0, col_major);
    DenseMatrix<int, double> *Br = B.transpose(), *Cr = C.transpose(); // row-major twins (before any GPU copy)
    A.sync2gpu(n_gpu, segment);
    B.sync2gpu(n_gpu, replicate);
    C.sync2gpu(n_gpu, replicate);
    Br->sync2gpu(n_gpu, replicate);
    Cr->sync2gpu(n_gpu, replicate);
    for (int call = 0; call < 2; ++call) {
        sblas_spmm_csr_v2<int, double>(&A, &B, &C, 3.0, 0.5, n_gpu);
        sblas_spmm_csr_v2<int, double>(&A, Br, Cr, 3.0, 0.5, n_gpu);
        CUDA_CHECK_ERROR();
        sblas_spmm_csr_cpu<int, double>(&A, &B, &C_cpu, 3.0, 0.5);
    }
    bool ok = true, same = true;
    const size_t h = (size_t)A.height, w = (size_t)b_width;
    for (unsigned i = 0; i < n_gpu; ++i) { // every GPU holds the full result
        C.sync2cpu(i);
        Cr->sync2cpu(i);
        const harness::Outcome o = harness::compare(C_cpu.val, C.val, C.get_mtx_num());
        bool bits = true;
        for (size_t r = 0; r < h && bits; ++r)
            for (size_t j = 0; j < w; ++j)
                if (memcmp(&Cr->val[r * w + j], &C.val[j * h + r], sizeof(double)) != 0) {
                    bits = false;
                    break;
                }
        printf("GPU %u: column-major %s (max rel err %.3g), row-major %s\n", i, o.correct ? "ok" : "MISMATCH", o.max_rel,
               bits ? "= transpose" : "DIFFERS");
        ok = ok && o.correct;
        same = same && bits;
    }
    delete Br;
    delete Cr;
    cout << "bit-identical: " << (same ? "yes" : "NO") << endl;
    cout << "order_test: " << (ok && same ? "PASS" : "FAIL") << endl;
    return ok && same ? 0 : 2;
}
