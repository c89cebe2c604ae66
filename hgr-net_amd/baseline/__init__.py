from .dgp import DGPTrainer, GCN_Dense_Att, GraphConv, GraphOperator, dropout_keep, fold_groups, group_edges
