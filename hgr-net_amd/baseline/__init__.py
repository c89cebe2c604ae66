from .dgp import DGPTrainer, GCN_Dense_Att, GraphConv, GraphOperator, dropout_keep, fold_groups, group_edges
from .dgp_eval import (DGPEvaluator, HostEvaluator, ListTree, build_list_tree, counters_host, load_features, load_pred, pick_vectors,
                       score_rows_host)
from .resnet import ResNet, ResNetBase, ResNetFeatures, make_resnet_base
from .cnzsl import CNZSLEvaluator, CNZSLModel, CNZSLTrainer, prototypes_host, score_host, train_step_host
from .free import (FR, Discriminator, Encoder, FREEClassifier, Generator, LinearLogSoftmaxClassifier, SynBatcher, features_host,
                   fit_step_host, fr_host, generator_host, make_opt, normal_host, synthesize, weights_init)
