"""The sparse updates a ``WideAndDeep`` holds between ``backward`` and
the apply, in one shape for both layouts of the tables."""


def sink_pairs(model):
    """``(deep, wide)``: two lists of ``(ids, grad)``, as they are pending
    now.  The replicated modules keep exactly these lists; the sharded
    module keeps one record per backward, read here as the deep and the
    wide pair of each record (both with the record's own ``ids``)."""
    if model.sharded:
        records = model.embeddings.pending_grads()
        return ([(r.ids, r.deep_grad) for r in records],
                [(r.ids, r.wide_grad) for r in records])
    return (model.deep_embedding.pending_grads(),
            model.wide_embedding.pending_grads())
