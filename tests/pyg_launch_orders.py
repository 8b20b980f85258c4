"""The recorded launches of tests/pyg_launch_cases.py (printed by `python tests/pyg_launch_cases.py`): per case the ordered
entry points of an eager run, or the name -> count dict of a captured step."""
ORDERS = {
    'GINEConv-h16-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_segment_pool_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32'
    ).split(),
    'GINEConv-h16-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_masked_linear_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32'
    ).split(),
    'GINEConv-h16-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_layers_f32 sn_gine_aggregate_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_gine_aggregate_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 '
        'sn_segment_pool_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_dot_finish_f64 sn_gine_aggregate_bwd_add_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_dot_finish_f64 sn_gine_aggregate_bwd_add_f32 sn_embedding_sum_bwd_layers_f32'
    ).split(),
    'GINEConv-h18-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_segment_pool_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32'
    ).split(),
    'GINEConv-h18-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_masked_linear_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32'
    ).split(),
    'GINEConv-h18-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_linear_bn_train_f32 '
        'sn_masked_affine_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_segment_pool_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gine_aggregate_bwd_f32 sn_bn_act_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_gine_aggregate_bwd_f32'
    ).split(),
    'GINConv-h16-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gin_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_gin_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_segment_pool_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32'
    ).split(),
    'GINConv-h16-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gin_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_masked_affine_f32 sn_gin_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_affine_f32 sn_masked_linear_f32'
    ).split(),
    'GINConv-h16-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gin_aggregate_f32 sn_masked_linear_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_gin_aggregate_f32 sn_masked_linear_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_segment_pool_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gin_aggregate_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gin_aggregate_f32'
    ).split(),
    'GINConv-h18-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gin_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_gin_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_segment_pool_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32'
    ).split(),
    'GINConv-h18-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gin_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_masked_affine_f32 sn_gin_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_affine_f32 sn_masked_linear_f32'
    ).split(),
    'GINConv-h18-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gin_aggregate_f32 sn_masked_linear_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_gin_aggregate_f32 sn_masked_linear_f32 sn_linear_bn_train_f32 '
        'sn_masked_affine_f32 sn_segment_pool_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gin_aggregate_f32 sn_bn_act_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gin_aggregate_f32'
    ).split(),
    'GCNConv-h16-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gcn_pyg_coef_f32 sn_gcn_pyg_propagate_f32 '
        'sn_masked_linear_f32 sn_gcn_pyg_propagate_f32 sn_masked_linear_f32 sn_segment_pool_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32'
    ).split(),
    'GCNConv-h16-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gcn_pyg_coef_f32 sn_gcn_pyg_propagate_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_gcn_pyg_propagate_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_affine_f32 sn_masked_linear_f32'
    ).split(),
    'GCNConv-h16-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gcn_pyg_coef_f32 sn_gcn_pyg_propagate_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_gcn_pyg_propagate_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_segment_pool_f32 sn_train_linear_f32 sn_train_bn_finish_f32 '
        'sn_train_bn_apply_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_train_bn_bwd_sums_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_bn_bwd_sums_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_gcn_pyg_propagate_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_gcn_pyg_propagate_f32'
    ).split(),
    'GCNConv-h18-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gcn_pyg_coef_f32 sn_gcn_pyg_propagate_f32 '
        'sn_masked_linear_f32 sn_gcn_pyg_propagate_f32 sn_masked_linear_f32 sn_segment_pool_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32'
    ).split(),
    'GCNConv-h18-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gcn_pyg_coef_f32 sn_gcn_pyg_propagate_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_gcn_pyg_propagate_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_affine_f32 sn_masked_linear_f32'
    ).split(),
    'GCNConv-h18-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gcn_pyg_coef_f32 sn_gcn_pyg_propagate_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_gcn_pyg_propagate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_segment_pool_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_gcn_pyg_propagate_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_gcn_pyg_propagate_f32'
    ).split(),
    'GATConv-h16-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_linear_f32'
    ).split(),
    'GATConv-h16-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32'
    ).split(),
    'GATConv-h16-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_gat_conv_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_bn_act_bwd_f32 '
        'sn_gat_conv_bwd_f32 sn_train_reduce_parts_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 '
        'sn_gat_conv_bwd_f32 sn_train_reduce_parts_f32 sn_masked_linear_f32 sn_linear_wgrad_f32'
    ).split(),
    'GATConv-h18-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_linear_f32'
    ).split(),
    'GATConv-h18-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32'
    ).split(),
    'GATConv-h18-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_gat_conv_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 sn_segment_pool_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_gat_conv_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_gat_conv_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_masked_linear_f32 sn_linear_wgrad_f32'
    ).split(),
    'SimplifiedPNAConv-h16-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_spna_mean_f32 '
        'sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_embedding_sum_f32 sn_masked_linear_f32 sn_spna_mean_f32 sn_masked_linear_f32 sn_embedding_sum_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32 sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_linear_f32'
    ).split(),
    'SimplifiedPNAConv-h16-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_spna_stats_f32 '
        'sn_spna_mean_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 '
        'sn_spna_stats_f32 sn_spna_mean_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32'
    ).split(),
    'SimplifiedPNAConv-h16-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 '
        'sn_spna_stats_f32 sn_spna_mean_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_train_linear_f32 sn_train_bn_finish_f32 '
        'sn_train_bn_apply_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_masked_linear_f32 '
        'sn_embedding_sum_f32 sn_masked_linear_f32 sn_spna_stats_f32 sn_spna_mean_f32 sn_masked_linear_f32 sn_embedding_sum_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_train_linear_f32 sn_train_bn_finish_f32 '
        'sn_train_bn_apply_f32 sn_segment_pool_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_spna_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_train_bn_bwd_sums_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_bn_bwd_sums_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_spna_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32'
    ).split(),
    'SimplifiedPNAConv-h18-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_spna_mean_f32 '
        'sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_embedding_sum_f32 sn_masked_linear_f32 sn_spna_mean_f32 sn_masked_linear_f32 sn_embedding_sum_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32 sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_linear_f32'
    ).split(),
    'SimplifiedPNAConv-h18-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_spna_stats_f32 '
        'sn_spna_mean_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 '
        'sn_spna_stats_f32 sn_spna_mean_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32'
    ).split(),
    'SimplifiedPNAConv-h18-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 '
        'sn_spna_stats_f32 sn_spna_mean_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 '
        'sn_spna_stats_f32 sn_spna_mean_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_spna_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_spna_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32'
    ).split(),
    'GINEConv-h16-mean-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_segment_pool_f32 '
        'sn_embedding_sum_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32'
    ).split(),
    'GCNConv-h18-mean-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gcn_pyg_coef_f32 sn_gcn_pyg_propagate_f32 '
        'sn_masked_linear_f32 sn_gcn_pyg_propagate_f32 sn_masked_linear_f32 sn_segment_pool_f32 sn_embedding_sum_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32'
    ).split(),
    'GINEConv-h16-pe-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_segment_pool_f32 sn_masked_linear_f32 sn_masked_linear_f32'
    ).split(),
    'GATConv-h16-pe-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_gat_conv_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32'
    ).split(),
    'GINEConv-h16-dropout-eval': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_segment_pool_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32'
    ).split(),
    'GINEConv-h16-mean-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_embedding_sum_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32'
    ).split(),
    'GCNConv-h18-mean-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gcn_pyg_coef_f32 sn_gcn_pyg_propagate_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_gcn_pyg_propagate_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_segment_pool_f32 sn_embedding_sum_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32'
    ).split(),
    'GINEConv-h16-pe-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_affine_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_affine_f32 sn_segment_pool_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_masked_linear_f32'
    ).split(),
    'GATConv-h16-pe-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_gat_conv_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_masked_linear_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32'
    ).split(),
    'GINEConv-h16-dropout-nograd': (
        'sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 sn_masked_affine_f32 '
        'sn_masked_linear_f32 sn_masked_affine_f32 sn_dropout_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_affine_f32 sn_dropout_f32 sn_segment_pool_f32 sn_masked_linear_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32'
    ).split(),
    'GINEConv-h16-mean-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_layers_f32 sn_gine_aggregate_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_gine_aggregate_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 '
        'sn_segment_pool_f32 sn_embedding_sum_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_train_bn_bwd_sums_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_bn_bwd_finish_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_dot_finish_f64 sn_gine_aggregate_bwd_add_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_dot_finish_f64 '
        'sn_gine_aggregate_bwd_add_f32 sn_embedding_sum_bwd_layers_f32'
    ).split(),
    'GCNConv-h18-mean-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gcn_pyg_coef_f32 sn_gcn_pyg_propagate_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_gcn_pyg_propagate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_segment_pool_f32 sn_embedding_sum_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_gcn_pyg_propagate_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_gcn_pyg_propagate_f32'
    ).split(),
    'GINEConv-h16-pe-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_layers_f32 sn_gine_aggregate_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 '
        'sn_gine_aggregate_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_linear_f32 sn_train_bn_finish_f32 '
        'sn_train_bn_apply_f32 sn_segment_pool_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_dot_finish_f64 sn_gine_aggregate_bwd_add_f32 sn_train_bn_bwd_sums_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_bn_bwd_finish_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_dot_finish_f64 sn_gine_aggregate_bwd_add_f32 '
        'sn_embedding_sum_bwd_layers_f32 sn_masked_linear_f32 sn_linear_wgrad_f32'
    ).split(),
    'GATConv-h16-pe-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 '
        'sn_gat_conv_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_gat_conv_f32 sn_masked_affine_f32 sn_segment_pool_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_bn_act_bwd_f32 sn_gat_conv_bwd_f32 sn_train_reduce_parts_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_gat_conv_bwd_f32 sn_train_reduce_parts_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32'
    ).split(),
    'GINEConv-h16-dropout-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_layers_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 '
        'sn_dropout_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_dropout_f32 sn_segment_pool_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_dropout_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_gine_aggregate_bwd_f32 sn_dropout_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_gine_aggregate_bwd_f32'
    ).split(),
    'GINEConv-h18-dropout-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_linear_bn_train_f32 '
        'sn_masked_affine_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_dropout_f32 sn_embedding_sum_f32 '
        'sn_gine_aggregate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_dropout_f32 sn_segment_pool_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_dropout_f32 sn_bn_act_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_gine_aggregate_bwd_f32 sn_dropout_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gine_aggregate_bwd_f32'
    ).split(),
    'SimplifiedPNAConv-h16-dropout-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 '
        'sn_spna_stats_f32 sn_spna_mean_f32 sn_masked_linear_f32 sn_embedding_sum_f32 sn_train_linear_f32 sn_train_bn_finish_f32 '
        'sn_train_bn_apply_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_dropout_f32 '
        'sn_masked_linear_f32 sn_embedding_sum_f32 sn_masked_linear_f32 sn_spna_stats_f32 sn_spna_mean_f32 sn_masked_linear_f32 '
        'sn_embedding_sum_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_dropout_f32 sn_segment_pool_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_dropout_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_spna_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_dropout_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_spna_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32'
    ).split(),
    'pyg.GNN-h16-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_layers_f32 sn_gine_aggregate_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_gine_aggregate_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 '
        'sn_segment_pool_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_dot_finish_f64 sn_gine_aggregate_bwd_add_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_dot_finish_f64 sn_gine_aggregate_bwd_add_f32 sn_embedding_sum_bwd_layers_f32'
    ).split(),
    'pyg.GNN-h16-l1-grad': (
        'sn_batch_plan sn_batch_plan sn_embedding_sum_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_segment_pool_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_dot_finish_f64 sn_gine_aggregate_bwd_add_f32'
    ).split(),
    'NetGINE-16-grad': (
        'sn_batch_plan sn_batch_plan sn_masked_linear_f32 sn_masked_linear_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_gine_aggregate_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_set2set_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_set2set_bwd_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gine_aggregate_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_gine_aggregate_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gine_aggregate_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_gine_aggregate_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_linear_wgrad_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gine_aggregate_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gine_aggregate_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_linear_wgrad_f32'
    ).split(),
    'SignNetGNN-gine-stages1-grad': (
        'sn_batch_plan sn_batch_plan sn_pack_eig_f32 sn_train_scalar_mlp_stats_f32 sn_gin_aggregate_f32 '
        'sn_train_scalar_mlp_stats_f32 sn_train_scalar_mlp_apply_f32 sn_gin_aggregate_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_masked_affine_f32 '
        'sn_train_linear_f32 sn_train_linear_f32 sn_train_linear_f32 sn_set_attention_f32 sn_train_linear_f32 '
        'sn_masked_layernorm_f32 sn_train_linear_f32 sn_train_linear_f32 sn_masked_layernorm_f32 sn_slot_sum_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_embedding_sum_f32 sn_masked_linear_f32 '
        'sn_embedding_sum_layers_f32 sn_gine_aggregate_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_gine_aggregate_f32 sn_train_linear_f32 sn_train_bn_finish_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_segment_pool_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_dot_finish_f64 '
        'sn_gine_aggregate_bwd_add_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_dot_finish_f64 sn_gine_aggregate_bwd_add_f32 sn_embedding_sum_bwd_layers_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_masked_layernorm_bwd_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_masked_layernorm_bwd_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_set_attention_bwd_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_dot_finish_f64 '
        'sn_gin_aggregate_add_f32 sn_train_scalar_mlp_bwd_f32'
    ).split(),
    'SignNetGNN-gine-stages0-grad': (
        'sn_batch_plan sn_batch_plan sn_pack_eig_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_linear_bn_train_f32 '
        'sn_masked_affine_f32 sn_gin_aggregate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_linear_bn_train_f32 '
        'sn_masked_affine_f32 sn_gin_aggregate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_linear_bn_train_f32 '
        'sn_masked_affine_f32 sn_gin_aggregate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_linear_bn_train_f32 '
        'sn_masked_affine_f32 sn_gin_aggregate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_linear_bn_train_f32 '
        'sn_masked_affine_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_set_attention_f32 sn_masked_linear_f32 sn_masked_layernorm_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_masked_layernorm_f32 sn_slot_sum_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_embedding_sum_f32 '
        'sn_masked_linear_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_embedding_sum_f32 sn_gine_aggregate_f32 sn_linear_bn_train_f32 '
        'sn_masked_affine_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_segment_pool_f32 sn_linear_bn_train_f32 '
        'sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gine_aggregate_bwd_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gine_aggregate_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_layernorm_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_layernorm_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_set_attention_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_affine_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_affine_f32 sn_bn_act_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gin_aggregate_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_affine_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gin_aggregate_f32 sn_bn_act_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32'
    ).split(),
    'SignNetGNN-alchemy-stages1-grad': (
        'sn_batch_plan sn_batch_plan sn_pack_eig_f32 sn_gin_aggregate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_gin_aggregate_f32 sn_linear_bn_train_f32 '
        'sn_masked_affine_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_gin_aggregate_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 '
        'sn_masked_affine_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_masked_affine_f32 sn_train_linear_f32 sn_train_linear_f32 sn_train_linear_f32 sn_set_attention_f32 '
        'sn_train_linear_f32 sn_masked_layernorm_f32 sn_train_linear_f32 sn_train_linear_f32 sn_masked_layernorm_f32 '
        'sn_train_linear_f32 sn_train_linear_f32 sn_train_linear_f32 sn_set_attention_f32 sn_train_linear_f32 '
        'sn_masked_layernorm_f32 sn_train_linear_f32 sn_train_linear_f32 sn_masked_layernorm_f32 sn_train_linear_f32 '
        'sn_train_linear_f32 sn_train_linear_f32 sn_set_attention_f32 sn_train_linear_f32 sn_masked_layernorm_f32 '
        'sn_train_linear_f32 sn_train_linear_f32 sn_masked_layernorm_f32 sn_train_linear_f32 sn_train_linear_f32 '
        'sn_train_linear_f32 sn_set_attention_f32 sn_train_linear_f32 sn_masked_layernorm_f32 sn_train_linear_f32 '
        'sn_train_linear_f32 sn_masked_layernorm_f32 sn_slot_sum_f32 sn_train_linear_f32 sn_train_bn_finish_f32 '
        'sn_train_bn_apply_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_gine_aggregate_f32 sn_train_linear_f32 sn_train_bn_finish_f32 '
        'sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_train_linear_f32 sn_train_bn_finish_f32 '
        'sn_train_bn_apply_f32 sn_gine_aggregate_f32 sn_train_linear_f32 sn_train_bn_finish_f32 sn_train_linear_f32 '
        'sn_train_bn_finish_f32 sn_train_bn_apply_f32 sn_segment_pool_f32 sn_train_linear_f32 sn_train_bn_finish_f32 '
        'sn_train_bn_apply_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_train_bn_bwd_sums_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_bn_bwd_sums_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_bn_bwd_finish_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_dot_finish_f64 sn_gine_aggregate_bwd_add_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_dot_finish_f64 '
        'sn_gine_aggregate_bwd_add_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_linear_wgrad_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_masked_layernorm_bwd_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_masked_layernorm_bwd_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_set_attention_bwd_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_masked_layernorm_bwd_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_masked_layernorm_bwd_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_set_attention_bwd_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_masked_layernorm_bwd_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_masked_layernorm_bwd_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_set_attention_bwd_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_masked_layernorm_bwd_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_masked_layernorm_bwd_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_set_attention_bwd_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_masked_affine_f32 '
        'sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_linear_wgrad_f32 '
        'sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_train_dot_finish_f64 '
        'sn_gin_aggregate_add_f32 sn_train_bn_bwd_sums_f32 sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 '
        'sn_train_reduce_parts_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_train_bn_bwd_sums_f32 '
        'sn_train_bn_bwd_finish_f32 sn_train_linear_bwd_f32 sn_train_reduce_parts_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32'
    ).split(),
    'SignNetGNN-alchemy-stages0-grad': (
        'sn_batch_plan sn_batch_plan sn_pack_eig_f32 sn_gin_aggregate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_gin_aggregate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_gin_aggregate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_gin_aggregate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_masked_affine_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_set_attention_f32 sn_masked_linear_f32 sn_masked_layernorm_f32 sn_masked_linear_f32 '
        'sn_masked_linear_f32 sn_masked_layernorm_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_set_attention_f32 sn_masked_linear_f32 sn_masked_layernorm_f32 sn_masked_linear_f32 sn_masked_linear_f32 '
        'sn_masked_layernorm_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_set_attention_f32 '
        'sn_masked_linear_f32 sn_masked_layernorm_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_layernorm_f32 '
        'sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_set_attention_f32 sn_masked_linear_f32 '
        'sn_masked_layernorm_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_masked_layernorm_f32 sn_slot_sum_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_masked_linear_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_gine_aggregate_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_gine_aggregate_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_linear_bn_train_f32 sn_masked_affine_f32 sn_segment_pool_f32 '
        'sn_linear_bn_train_f32 sn_masked_affine_f32 sn_masked_linear_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gine_aggregate_bwd_f32 sn_bn_act_bwd_f32 '
        'sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_gine_aggregate_bwd_f32 sn_bn_act_bwd_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_layernorm_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_layernorm_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_set_attention_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_layernorm_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_layernorm_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_set_attention_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_layernorm_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_layernorm_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_set_attention_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_layernorm_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_layernorm_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_set_attention_bwd_f32 sn_masked_linear_f32 '
        'sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_affine_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_linear_wgrad_f32 '
        'sn_masked_affine_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_masked_affine_f32 sn_bn_act_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gin_aggregate_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 '
        'sn_masked_affine_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32 sn_gin_aggregate_f32 sn_bn_act_bwd_f32 '
        'sn_masked_linear_f32 sn_linear_wgrad_f32 sn_bn_act_bwd_f32 sn_masked_linear_f32 sn_linear_wgrad_f32'
    ).split(),
    'captured-SimplifiedPNAConv-h16': {'sn_batch_plan': 6, 'sn_bucket_pack': 1, 'sn_embedding_sum_f32': 15, 'sn_linear_wgrad_f32': 21, 'sn_masked_affine_f32': 6, 'sn_masked_l1_bwd_f32': 3, 'sn_masked_l1_f32': 3, 'sn_masked_linear_f32': 42, 'sn_segment_pool_f32': 3, 'sn_spna_bwd_masked_f32': 6, 'sn_spna_mean_f32': 6, 'sn_spna_stats_masked_f32': 6, 'sn_train_bn_apply_f32': 15, 'sn_train_bn_bwd_sums_f32': 15, 'sn_train_bn_finish_f32': 15, 'sn_train_linear_bwd_f32': 15, 'sn_train_linear_f32': 15, 'sn_train_reduce_jobs_f32': 3},
    'captured-NetGINE-16': {'sn_batch_plan': 6, 'sn_bucket_pack': 1, 'sn_gine_aggregate_bwd_f32': 18, 'sn_gine_aggregate_f32': 18, 'sn_linear_wgrad_f32': 81, 'sn_masked_affine_f32': 3, 'sn_masked_l1_bwd_f32': 3, 'sn_masked_l1_f32': 3, 'sn_masked_linear_f32': 138, 'sn_set2set_bwd_f32': 3, 'sn_set2set_f32': 3},
}
