// sddmm_test -- sblas_sddmm_csr (the values of A on its own pattern from dense X and Y) on <gpus> GPUs and on one, in the
// four order combinations of X and Y, each against the host verifier.  Every combination and every GPU count must give
// the same bits: the summation order of an entry depends on k alone.   sddmm_test <matrix.mtx> <gpus> [k]
#include <cstring>
#include <vector>

#include "harness.h"

static std::vector<double> run(const char *path, DenseMatrix<int, double> *X, DenseMatrix<int, double> *Y, unsigned n_gpu,
                               double alpha, double beta)
{
    CsrSparseMatrix<int, double> A(path);
    A.sync2gpu(n_gpu, segment);
    sblas_sddmm_csr<int, double>(&A, X, Y, alpha, beta, n_gpu);
    CUDA_CHECK_ERROR();
    return std::vector<double>(A.csrVal, A.csrVal + A.nnz);
}

int main(int argc, char *argv[])
{
    if (argc < 3) {
        cerr << "usage: sddmm_test <matrix.mtx> <gpus> [k]" << endl;
        return 1;
    }
    const unsigned n_gpu = (unsigned)atoi(argv[2]);
    const int k = argc > 3 ? atoi(argv[3]) : 64;
    CsrSparseMatrix<int, double> A_cpu(argv[1]);
    if (A_cpu.height == 0 || A_cpu.nnz == 0 || k <= 0 || n_gpu == 0) return 1;
    const double alpha = 3.0, beta = 0.5;
    DenseMatrix<int, double> Xc(A_cpu.height, k, col_major), Yc(A_cpu.width, k, col_major);
    for (size_t i = 0; i < Yc.get_mtx_num(); ++i) Yc.val[i] = 1.0 - 0.5 * Yc.val[i]; // not X's values again
    DenseMatrix<int, double> *Xr = Xc.transpose(), *Yr = Yc.transpose();               // row-major twins
    sblas_sddmm_csr_cpu<int, double>(&A_cpu, &Xc, &Yc, alpha, beta);
    DenseMatrix<int, double> *Xs[2] = {&Xc, Xr}, *Ys[2] = {&Yc, Yr};
    for (int o = 0; o < 2; ++o) {
        Xs[o]->sync2gpu(n_gpu, replicate);
        Ys[o]->sync2gpu(n_gpu, replicate);
    }
    bool ok = true, same = true;
    std::vector<double> first;
    for (int ox = 0; ox < 2; ++ox)
        for (int oy = 0; oy < 2; ++oy) {
            const std::vector<double> many = run(argv[1], Xs[ox], Ys[oy], n_gpu, alpha, beta);
            const std::vector<double> one = n_gpu > 1 ? run(argv[1], Xs[ox], Ys[oy], 1, alpha, beta) : many;
            const harness::Outcome o = harness::compare(A_cpu.csrVal, many.data(), many.size());
            const bool bits = memcmp(one.data(), many.data(), many.size() * sizeof(double)) == 0;
            if (first.empty()) first = many;
            const bool orders = memcmp(first.data(), many.data(), many.size() * sizeof(double)) == 0;
            printf("X %s, Y %s: %s (max rel err %.3g), %u GPUs %s one GPU, orders %s\n", ox ? "row-major" : "column-major",
                   oy ? "row-major" : "column-major", o.correct ? "ok" : "MISMATCH", o.max_rel, n_gpu, bits ? "=" : "DIFFER FROM",
                   orders ? "agree" : "DIFFER");
            ok = ok && o.correct;
            same = same && bits && orders;
        }
    delete Xr;
    delete Yr;
    cout << "bit-identical: " << (same ? "yes" : "NO") << endl;
    cout << "sddmm_test: " << (ok && same ? "PASS" : "FAIL") << endl;
    return ok && same ? 0 : 2;
}
