"""Requests that share a launch on the MI355X: the segmented IDF mapping against requests sent alone — bit for bit in all three pool
forms —, batch_requests / score_requests against the per-request path, and the graphs by bucket: one captured chain per power of two
serves every request mix and every padded total of its bucket, before and after the pool and the weights change."""
import pytest

import online_requests_cases as qc

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


@pytest.mark.parametrize("form", qc.FORMS)
def test_segmented_retrieve_equals_requests_sent_alone_gpu(form):
    qc.check_retrieval_parity("tiny_seq_bn", 0, _lib(), form, splits=(1, 3, 7, 0))


def test_segmented_retrieve_300_row_pool_gpu():
    qc.check_retrieval_parity("tiny_seq_bn", 0, _lib(), "immutable", splits=(1, 7, 64), n_pool=300)


@pytest.mark.parametrize("form", qc.FORMS)
def test_batch_and_score_requests_equal_requests_sent_alone_gpu(form):
    qc.check_assembly_and_prediction("tiny_seq_bn", 0, _lib(), form)


@pytest.mark.parametrize("form", qc.FORMS)
def test_bucket_graphs_serve_every_mix_and_survive_pool_changes_gpu(form):
    qc.check_bucket_graphs("tiny_seq_bn", 0, _lib(), form)


def test_request_refusals_gpu():
    qc.check_request_refusals(0, _lib())
