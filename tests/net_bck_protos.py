"""The two tiny nets of the backward net-run tests: batch 2, 3 x 19 x 19 input, 5 classes. Neither pool
follows a ReLU or another pool, so with random inputs no window has two equal maxima and tied maxima cannot
decide a gradient."""


def _data():
    return ('layer { name: "data" type: "Data" top: "data" top: "label"\n'
            '  transform_param { crop_size: 19 } data_param { batch_size: 2 } }\n')


def _conv(name, bot, n, k, pad=0, relu=True):
    s = ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s"\n'
         '  convolution_param { num_output: %d kernel_size: %d pad: %d } }\n' % (name, bot, name, n, k, pad))
    if relu:
        s += 'layer { name: "%s_relu" type: "ReLU" bottom: "%s" top: "%s" }\n' % (name, name, name)
    return s


def _tail(bot):
    return ('layer { name: "gpool" type: "Pooling" bottom: "%s" top: "gpool"\n'
            '  pooling_param { pool: AVE global_pooling: true } }\n'
            'layer { name: "loss" type: "SoftmaxWithLoss" bottom: "gpool" bottom: "label" top: "loss" }\n' % bot)


# conv3x3 + ReLU -> LRN -> maxpool 3x3 s2 -> conv1x1 + ReLU -> dropout -> global avgpool -> loss
CHAIN = ('name: "chain"\n' + _data() + _conv("conv1", "data", 8, 3) +
         'layer { name: "norm1" type: "LRN" bottom: "conv1" top: "norm1"\n'
         '  lrn_param { local_size: 5 alpha: 0.01 beta: 0.75 } }\n'
         'layer { name: "pool1" type: "Pooling" bottom: "norm1" top: "pool1"\n'
         '  pooling_param { pool: MAX kernel_size: 3 stride: 2 } }\n' + _conv("conv2", "pool1", 5, 1) +
         'layer { name: "drop" type: "Dropout" bottom: "conv2" top: "conv2" dropout_param { dropout_ratio: 0.5 } }\n' +
         _tail("conv2"))

# one blob feeding a 1x1 conv, a 3x3 p1 conv and a 3x3 s1 p1 maxpool -> 1x1 conv, all into Concat,
# then conv1x1 -> global avgpool -> loss
INCEPTION = ('name: "inception"\n' + _data() + _conv("stem", "data", 6, 3, relu=False) +
             _conv("b1", "stem", 4, 1) + _conv("b2", "stem", 4, 3, pad=1) +
             'layer { name: "bpool" type: "Pooling" bottom: "stem" top: "bpool"\n'
             '  pooling_param { pool: MAX kernel_size: 3 stride: 1 pad: 1 } }\n' + _conv("b3", "bpool", 4, 1) +
             'layer { name: "cat" type: "Concat" bottom: "b1" bottom: "b2" bottom: "b3" top: "cat" }\n' +
             _conv("cls", "cat", 5, 1, relu=False) + _tail("cls"))
