"""GPU: k_zklaim_witness alone (zkg_zklaim_witness_gpu) against the host witness pass — tags, listed indices and listed values byte for
byte, for every credential of zklaim_witness_cases, in batches of 1, 3 and 16 contexts."""
import pytest

from gpu_util import zkg  # noqa: F401
from zklaim_witness_cases import N_SPECS, assert_same_witness, host_pass, payloads

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 8]


@pytest.mark.parametrize("k", KS)
def test_generator_equals_host_pass(zkg, k):
    keep = []
    ctxs = [zkg.make_ctx(payloads(k, j % N_SPECS, j // N_SPECS), keep) for j in range(16)]
    want = [host_pass(zkg, c) for c in ctxs]
    assert len({w[1].size for w in want}) >= 2
    for batch in ([9], [0, 7, 8], [3], list(range(16))):                      # 1, 3, 1 and 16 contexts: every spec is in one of them
        got = zkg.zklaim_witness_gpu([ctxs[j] for j in batch])
        assert len(got) == len(batch)
        for j, g in zip(batch, got):
            assert_same_witness(g, want[j], (k, j, len(batch)))
    for j in range(N_SPECS):                                                   # and every spec alone
        assert_same_witness(zkg.zklaim_witness_gpu([ctxs[j]])[0], want[j], (k, j, "alone"))


@pytest.mark.parametrize("k", [1, 3])
def test_bad_contexts_fail_alone(zkg, k):
    keep = []
    good = [zkg.make_ctx(payloads(k, j), keep) for j in range(4)]
    other = zkg.make_ctx(payloads(k + 1, 2), keep)                             # another payload count than the batch's
    broken = zkg.make_ctx(payloads(k, 5), keep)
    broken.pl_ctx_head = None                                                  # the list is shorter than num_of_payloads says
    batch = [good[0], None, good[1], other, good[2], broken, good[3]]
    got = zkg.zklaim_witness_gpu(batch)
    assert [g is None for g in got] == [False, True, False, True, False, True, False]
    for j, at in enumerate((0, 2, 4, 6)):
        assert_same_witness(got[at], host_pass(zkg, good[j]), (k, j))
