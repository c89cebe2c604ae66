"""Host-only: the guard in front of OMTrainer's gather / scatter loop.  hgr_rows_axpy is a plain ``+=`` per destination row, so the
ids of one inner step must be distinct; the check is a pure function of the host lists (no library, no device)."""
import pytest

from hgr_net_amd import training


def test_check_distinct_ids_names_the_duplicate():
    training.check_distinct_ids([])
    training.check_distinct_ids([[3, 1, 2], [1, 2, 3], [7]])             # the same node in DIFFERENT steps is the normal case
    with pytest.raises(ValueError, match=r"inner step 1 lists node 5 twice"):
        training.check_distinct_ids([[0, 1, 2], [4, 5, 6, 5], [9, 9]])     # the first offender is named


def test_train_batch_checks_picks_before_the_scatter_loop():
    """train_batch calls the guard on the picks it is about to use, before the text tower and the loop of rows_gather / rows_axpy."""
    import inspect
    src = inspect.getsource(training.OMTrainer.train_batch)
    at = src.index("check_distinct_ids(")
    assert at < src.index("text_fwd(") and at < src.index("ops.rows_gather(") and at < src.index("ops.rows_axpy(")
    assert at > src.index("get_contra_ids(")                               # ... and after they were drawn (and agreed on across ranks)
    assert at > src.index("_agree_on_picks(")
