from .moe import moe_combine, moe_dispatch, sort_by_expert, topk_route  # noqa: F401
