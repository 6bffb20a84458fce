from .evaluation import EvalResult, all_reduce_result, eval_shard, evaluate
from .fused_step import FusedSimpleCNNEngine, EngineOptions
from .graph_step import GraphedStep

__all__ = ["FusedSimpleCNNEngine", "EngineOptions", "GraphedStep", "EvalResult", "all_reduce_result",
           "eval_shard", "evaluate"]
