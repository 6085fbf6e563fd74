"""_native.workspace, the one workspace idiom of the op modules, at its edges: the zero fill that mm_attribute_loss_* and mm_mesh_reg_* take
as their ABI contract must happen on a block the caching allocator hands back dirty, and a zero-byte query (mm_ssim_*) must give a
non-NULL pointer of at least one byte while workspace_bytes stays what the library said."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def test_workspace_zero_fill_and_zero_byte_query(pkg):
    N = pkg._native
    d = N.MMAttLossDesc()
    d.B, d.V, d.Ht, d.Wt = 1, 1, 1, 1
    nbytes = N.fn("mm_attribute_loss_query_workspace")(d)
    assert nbytes > 0
    dirty = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    block = dirty.data_ptr()
    del dirty                                                     # (back to the caching allocator, which hands the same block out next)
    t = N.workspace("mm_attribute_loss_query_workspace", d, DEV, zero=True)
    print("queried %d bytes; block reused: %s" % (nbytes, t.data_ptr() == block))
    assert t.dtype == torch.uint8 and t.numel() == nbytes and t.device == DEV
    assert int(t.max()) == 0
    assert d.workspace == t.data_ptr() and d.workspace_bytes == nbytes

    s = N.MMSsimDesc()                                            # all-zero: the query answers 0
    assert N.fn("mm_ssim_query_workspace")(s) == 0
    t1 = N.workspace("mm_ssim_query_workspace", s, DEV, zero=False, at_least=1)
    assert t1.dtype == torch.uint8 and t1.numel() == 1
    assert s.workspace is not None and s.workspace == t1.data_ptr() != 0
    assert s.workspace_bytes == 0
