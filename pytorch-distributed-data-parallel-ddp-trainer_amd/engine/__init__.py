from .evaluation import (EvalResult, ResNetEvaluator, all_reduce_result, eval_shard, evaluate,
                         evaluate_resnet)
from .fused_step import FusedSimpleCNNEngine, EngineOptions
from .graph_step import GraphedStep

__all__ = ["FusedSimpleCNNEngine", "EngineOptions", "GraphedStep", "EvalResult", "all_reduce_result",
           "eval_shard", "evaluate", "evaluate_resnet", "ResNetEvaluator"]
